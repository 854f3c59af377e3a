"""k-nearest closest-point queries on the device (rt_closest_points_multi[_device], k_nearest<2 / 4 / 8>): the device form and the host
form against rt_scene_nearest_host(use_bvh = 0) on the same scene object and, on the three small scenes, against the numpy model
(tests/nearest_scenes.py; tests/test_nearest.py holds the host brute force to it without a GPU). Every comparison is bit for bit."""
import numpy as np
import pytest

import closest_scenes as cs
import nearest_scenes as ns
from nearest_scenes import OUTPUTS, SLOTS, key_mix, nearest_model, same, small_case
from rtamd import abi, scenes
from rtamd.renderer import Scene
from test_closest_points import NO_TRI, point_mix

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    return 0


def near_dev(s, pos, k, max_dist2=None, after=None, stream=None, outputs=OUTPUTS, canary=7):
    """rt_closest_points_multi_device on torch tensors (max_dist2 SQUARED); returns numpy results (outputs not asked for keep the canary)"""
    import torch
    n = len(pos)
    up = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()  # (a copy: the shared points are read-only)
    p = up(pos, f32)
    md = up(max_dist2, f32) if max_dist2 is not None else None
    ad, atri = (up(after[0], f32), up(np.asarray(after[1], np.uint32).view(np.int32), np.int32)) if after is not None else (None, None)
    st = stream or torch.cuda.current_stream()
    bufs = {name: torch.full((n,) if name == "count" else (n, k), canary, dtype=torch.int32 if name in ("tri", "count") else torch.float32, device="cuda")
            for name in OUTPUTS}
    torch.cuda.synchronize()
    s.closest_points_multi_device(n, k, p.data_ptr(), d_max_dist2=md.data_ptr() if md is not None else 0,
                                  d_after_dist2=ad.data_ptr() if ad is not None else 0, d_after_tri=atri.data_ptr() if atri is not None else 0,
                                  stream=st.cuda_stream, **{"d_" + name: bufs[name].data_ptr() for name in outputs})
    st.synchronize()
    out = {name: bufs[name].cpu().numpy() for name in OUTPUTS}
    out["tri"], out["count"] = out["tri"].view(np.uint32), out["count"].view(np.uint32)
    return out


def host_form(s, pos, k, max_dist2=None, after=None):
    """rt_closest_points_multi with SQUARED radii (Scene.closest_points_multi squares a radius; the tests' radii are squared already,
    negative ones among them) -> the outputs without "dist\""""
    out = s._nearest_call(np.ascontiguousarray(pos, f32), k, None if max_dist2 is None else np.ascontiguousarray(max_dist2, f32),
                          (None, None) if after is None else (np.ascontiguousarray(after[0], f32), np.ascontiguousarray(after[1], np.uint32)))
    return {name: out[name] for name in OUTPUTS}


def hold(s, pos, k, what, max_dist2=None, after=None, model=None):
    """device form == host form == nearest_host(use_bvh = 0) on the same scene (== `model` where given) -> the brute force's result"""
    want = s.nearest_host(pos, k, max_dist2, after)
    if model is not None:
        same(want, model, f"{what}: brute force vs model")
    same(near_dev(s, pos, k, max_dist2, after), want, f"{what}: device")
    same(host_form(s, pos, k, max_dist2, after), want, f"{what}: host form")
    return want


# ---- the three small scenes, against the model ----------------------------------------------------------------------------------------------
def test_cornell_equals_the_model_at_every_size(gpu):
    """n = 1, 63, 64, 65 and 513 (one lane, a wave less one, a wave, a wave and one, a workgroup and one) and 2,000; k = 1, 2, 4 and 8 (the
    three instantiations), free and under the radius and key mix; and the public wrapper's radius, squared in fp32."""
    c = small_case("cornell")
    s = Scene(c["sd"], device=gpu)
    free = nearest_model(c["table"], 8)
    md2, after = key_mix(free, 3)
    for n in (1, 63, 64, 65, 513, 2000):
        tab = {name: a[:, :n] for name, a in c["table"].items()}
        pos = c["pos"][:n]
        for k in (1, 2, 8):
            hold(s, pos, k, f"cornell n={n} k={k}", model=nearest_model(tab, k))
        mix = (md2[:n], (after[0][:n], after[1][:n]))
        hold(s, pos, 4, f"cornell n={n} k=4 mix", *mix, model=nearest_model(tab, 4, *mix))
    n = len(c["pos"])
    got = s.closest_points_multi(c["pos"], 8, f32(0.25 * c["scale"]))
    want = nearest_model(c["table"], 8, ns.squared_radius(c["scale"], 0.25, n))
    same(got, want, "cornell within 0.25 scales, the wrapper")
    np.testing.assert_array_equal(got["dist"], np.sqrt(want["dist2"]))
    assert (want["count"] == 8).mean() >= 0.3 and (want["count"] == 0).any()
    s.close()


@pytest.mark.parametrize("k", range(1, 9))
def test_ties_across_the_last_slot_on_the_duplicates(gpu, k):
    """Seven shuffled cubes: in one of the two runs of every k (nearest_scenes.duplicate_runs) a tie straddles slot k - 1 on every point —
    the entry that stays is the one with the lower index, and the box at the bound's distance is entered."""
    c = small_case("duplicates")
    s = Scene(c["sd"], device=gpu)
    for what, after in ns.duplicate_runs(c["table"], k):
        hold(s, c["pos"], k, f"duplicates k={k} {what}", None, after, model=nearest_model(c["table"], k, None, after))
    s.close()


def test_every_instantiation_is_reached_and_the_wrong_one_would_fail(gpu):
    """The pile of 256, every point with 256 counting triangles: k = 3 (a 2-slot list could not hold them, a bound on the wrong slot would
    keep the fourth), k = 5 .. 8 (a 4-slot list could not), and k = 2 / 4 / 8 at the top of each list; every list is full."""
    c = small_case("pile256")
    s = Scene(c["sd"], device=gpu)
    for k in (2, 3, 4, 5, 6, 7, 8):
        want = hold(s, c["pos"], k, f"pile256 k={k}", model=nearest_model(c["table"], k))
        assert (want["count"] == k).all()
    free = nearest_model(c["table"], 8)
    md2, after = key_mix(free, 4)
    hold(s, c["pos"], 3, "pile256 k=3 mix", md2, after, model=nearest_model(c["table"], 3, md2, after))
    hold(s, c["pos"], 7, "pile256 k=7 mix", md2, after, model=nearest_model(c["table"], 7, md2, after))
    s.close()


# ---- refills beside live lanes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3])
def test_waves_refill_beside_live_lanes(gpu, devlib, monkeypatch, grid):
    """5,000 points of the Cornell box under RT_NEAREST_GRID = 1 and 3 (the developer build's knob, read at a scene's first launch of an
    instantiation): one or three workgroups claim the whole list, so every wave opens new lists beside lanes that hold full ones; with
    the radius and key mix many entries end at the root."""
    monkeypatch.setenv("RT_NEAREST_GRID", str(grid))
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=gpu, lib=devlib)
    pos = point_mix(sd, 5000, 17)
    free = hold(s, pos, 8, f"grid {grid}")
    md2, after = key_mix(free, 5)
    for k in (2, 3, 8):
        hold(s, pos, k, f"grid {grid} k={k} mix", md2, after)
    s.close()


# ---- deep stacks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh", "lbvh_gpu"])
def test_the_full_pile_spills_the_stack_under_a_moving_bound(gpu, devlib, monkeypatch, builder):
    """8,192 parallel triangles in one box: stack_need > kLdsStack on the very tree the kernel walks, so lanes push and pop through the
    spill routines while their bound moves. k = 8 and k = 3 on 1,024 points. Then one wave (n = 64 under RT_NEAREST_GRID=1) whose even
    entries have max_dist2 = -1 — the root is visited, nothing is entered, the sentinel is popped — and whose odd entries are unbounded."""
    sd = cs.pile_scene()
    s = Scene(sd, gpu, cs.BUILDERS[builder], lib=devlib)
    tree = s.tree()
    assert tree["stack_need"] > cs.K_LDS_STACK and tree["built_by"] == cs.BUILDERS[builder]
    pos = np.concatenate([point_mix(sd, 768, 1), cs.pile_corner_points(256, 2)])
    want = hold(s, pos, 8, f"pile {builder} k=8")
    assert (want["count"] == 8).all()
    hold(s, pos, 3, f"pile {builder} k=3")
    s.close()
    monkeypatch.setenv("RT_NEAREST_GRID", "1")
    s = Scene(sd, gpu, cs.BUILDERS[builder], lib=devlib)
    assert s.tree()["stack_need"] > cs.K_LDS_STACK
    md2 = np.where(np.arange(64) % 2 == 0, f32(-1.0), f32(np.inf)).astype(f32)
    want = s.nearest_host(pos[:64], 8, md2)
    assert (want["count"][0::2] == 0).all() and (want["count"][1::2] == 8).all()
    same(near_dev(s, pos[:64], 8, md2), want, f"pile {builder}: one wave, shallow and spilled lanes")
    s.close()


# ---- de-duplication and NaN candidates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh", "lbvh_gpu"])
def test_the_mixed_scene_lists_pre_split_triangles_once(gpu, builder):
    """Two scene-spanning triangles (pre-split under SAH: whole in many leaves) over 3,000 tiny ones, 500 slivers and 300 degenerate
    triangles, 100 of which give NaN candidates, against the host brute force over the triangle list: equality on every one of 2,048
    points, free and under the radius and key mix — this query has no conditioning limit. No list holds an index twice or a NaN."""
    sd, _ = cs.mixed_scene()
    s = Scene(sd, gpu, cs.BUILDERS[builder])
    assert (s.info().n_split_triangles > 0) == (builder == "sah")
    pos = point_mix(sd, 2048, 7)
    want = hold(s, pos, 8, f"mixed {builder} k=8")
    srt = np.sort(want["tri"], 1)
    assert not (srt[:, 1:] == srt[:, :-1]).any() and (want["count"] == 8).all() and not np.isnan(want["dist2"]).any()
    md2, after = key_mix(want, 9)
    for k in (1, 2, 4):
        hold(s, pos, k, f"mixed {builder} k={k}")
        hold(s, pos, k, f"mixed {builder} k={k} mix", md2, after)
    s.close()


# ---- real trees -------------------------------------------------------------------------------------------------------------------------------
TREES = {
    "atrium_sah": lambda gpu: Scene(scenes.get_scene("atrium", detail=1), gpu, abi.RT_BVH_SAH),
    "atrium_lbvh_gpu": lambda gpu: Scene(scenes.get_scene("atrium", detail=1), gpu, abi.RT_BVH_LBVH_GPU),
    "tilted_sah": lambda gpu: Scene(scenes.atrium_tilted_scene(1), gpu, abi.RT_BVH_SAH),
}


@pytest.mark.parametrize("case", sorted(TREES))
def test_the_atrium(gpu, case):
    import torch
    s = TREES[case](gpu)
    pos = point_mix(s.desc, 1024, 19)
    n = len(pos)
    want = hold(s, pos, 8, f"{case} k=8")
    assert (want["count"] == 8).all()
    md2, after = key_mix(want, 4)
    hold(s, pos, 4, f"{case} k=4 mix", md2, after)
    one = hold(s, pos, 1, f"{case} k=1")
    # the k = 1 identity on the device: rt_closest_points_device bit for bit
    p = torch.from_numpy(pos).cuda()
    bufs = {k: torch.full((n,), 7, dtype=torch.int32 if k == "tri" else torch.float32, device="cuda") for k in SLOTS}
    torch.cuda.synchronize()
    s.closest_points_device(n, p.data_ptr(), **{"d_" + k: bufs[k].data_ptr() for k in SLOTS})
    torch.cuda.synchronize()
    for k in SLOTS:
        np.testing.assert_array_equal(bufs[k].cpu().numpy().view(np.uint32), one[k][:, 0].view(np.uint32), err_msg=k)
    s.close()


def test_an_updated_scene_equals_a_fresh_build(gpu):
    from test_scene_update import update_sequence
    sd = scenes.get_scene("atrium", detail=1)
    s = Scene(sd, gpu, abi.RT_BVH_LBVH, updatable=True)
    pos = point_mix(sd, 1024, 23)
    before = near_dev(s, pos, 8)
    for u in update_sequence(sd)[:2]:
        s.update(**u)
    fresh = Scene(s.desc, gpu, abi.RT_BVH_LBVH)
    want = hold(fresh, pos, 8, "fresh build")
    same(near_dev(s, pos, 8), want, "updated scene")
    same(s.nearest_host(pos, 8, use_bvh=True), want, "updated scene, host walk")
    assert not np.array_equal(before["dist2"], want["dist2"])
    s.close(), fresh.close()


# ---- paging on the device -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "pile256"])
def test_pages_of_two_fed_back_on_the_device_equal_one_call_of_eight(gpu, name):
    """Four pages of 2, each continued from the DEVICE buffers of the one before — the key is the page's last slot, gathered by a device
    copy on the same stream, no host round trip and no synchronisation between the pages. Within 0.25 scene scales many points of the
    Cornell box are exhausted early: their last slot is the miss, (+inf, 0xFFFFFFFF), a key behind which nothing counts."""
    import torch
    c = small_case(name)
    s = Scene(c["sd"], device=gpu)
    n = len(c["pos"])
    md2 = ns.squared_radius(c["scale"], 0.25, n)
    p, md = torch.from_numpy(np.array(c["pos"])).cuda(), torch.from_numpy(md2).cuda()
    st = torch.cuda.Stream(device=0)
    pages = [{k: torch.full((n, 2), 7, dtype=torch.int32 if k == "tri" else torch.float32, device="cuda") for k in SLOTS} for _ in range(4)]
    counts = [torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ad = atri = None
        for pg, cnt in zip(pages, counts):
            s.closest_points_multi_device(n, 2, p.data_ptr(), d_max_dist2=md.data_ptr(), d_after_dist2=ad.data_ptr() if ad is not None else 0,
                                          d_after_tri=atri.data_ptr() if atri is not None else 0, d_count=cnt.data_ptr(), stream=st.cuda_stream,
                                          **{"d_" + k: pg[k].data_ptr() for k in SLOTS})
            ad, atri = pg["dist2"][:, 1].contiguous(), pg["tri"][:, 1].contiguous()
    st.synchronize()
    got = {k: np.concatenate([pg[k].cpu().numpy() for pg in pages], 1) for k in SLOTS}
    got["tri"] = got["tri"].view(np.uint32)
    got["count"] = sum(cnt.cpu().numpy().view(np.uint32) for cnt in counts)
    want = nearest_model(c["table"], 8, md2)
    same(got, want, f"{name} pages of 2 on the device")
    same(got, s.nearest_host(c["pos"], 8, md2), f"{name} pages of 2 vs the brute force")
    if name == "cornell":
        assert (want["count"] < 8).mean() > 0.5 and (want["count"] == 8).mean() >= 0.3
    s.close()


# ---- rejected entries, NULL outputs ------------------------------------------------------------------------------------------------------------
def test_rejected_entries_are_marked_and_the_rest_answered(gpu):
    """The device form marks exactly the entries the host form refuses one by one: a point outside the contract range, a non-finite
    point, a NaN max_dist2, a NaN after_dist2 — every slot dist2 = NaN and tri = RT_TRI_REJECTED, u and v unwritten, count = 0."""
    c = small_case("cornell")
    s = Scene(c["sd"], device=gpu)
    n, k = 256, 3
    pos = c["pos"][:n].copy()
    free = nearest_model({name: a[:, :n] for name, a in c["table"].items()}, 8)
    md2, after = key_mix(free, 6)
    ad, atri = after[0].copy(), after[1].copy()
    _, _, limit = cs.contract_limits(c["sd"])
    pos[5, 0] = np.nan
    pos[70, 2] = np.inf
    pos[131] = np.array([1.0, 1.0, 1.0], f32) * f32(103.0) * limit / f32(100.0) + f32(3.0) * limit
    md2[9] = np.nan
    ad[200] = np.nan
    bad = np.zeros(n, bool)
    bad[[5, 9, 70, 131, 200]] = True
    got = near_dev(s, pos, k, md2, (ad, atri), canary=7)
    assert np.isnan(got["dist2"][bad]).all() and (got["tri"][bad] == abi.RT_TRI_REJECTED).all() and (got["count"][bad] == 0).all()
    assert (got["u"][bad] == 7).all() and (got["v"][bad] == 7).all()
    want = s.nearest_host(pos[~bad], k, md2[~bad], (ad[~bad], atri[~bad]))
    same({name: a[~bad] for name, a in got.items()}, want, "accepted entries")
    same(host_form(s, pos[~bad], k, md2[~bad], (ad[~bad], atri[~bad])), want, "accepted entries, host form")
    for i in np.flatnonzero(bad):  # the host form refuses each of them alone, naming it, and writes nothing
        one = slice(i, i + 1)
        with pytest.raises(abi.RtError) as e:
            host_form(s, pos[one], k, md2[one], (ad[one], atri[one]))
        assert e.value.status == abi.RT_ERR_INVALID and "point 0" in str(e.value), i
    for i in np.flatnonzero(~bad)[:4]:
        one = slice(i, i + 1)
        host_form(s, pos[one], k, md2[one], (ad[one], atri[one]))
    s.close()


def test_null_outputs_are_left_alone(gpu):
    c = small_case("cornell")
    s = Scene(c["sd"], device=gpu)
    want = nearest_model(c["table"], 4)
    for outputs in (("dist2",), ("tri", "count"), ("count",), ("u", "v")):
        got = near_dev(s, c["pos"], 4, outputs=outputs, canary=7)
        for name in OUTPUTS:
            if name in outputs:
                np.testing.assert_array_equal(got[name].view(np.uint32), want[name].view(np.uint32), err_msg=str(outputs))
            else:
                assert (got[name] == 7).all(), (outputs, name)
    s.close()


def test_a_nearest_query_and_a_multihit_query_on_two_streams_without_host_synchronisation(gpu, scene_cache):
    """The two launches share the scene's cursors: the later waits for the earlier on the device. Nothing synchronises between the
    enqueues; one synchronisation at the end."""
    import torch
    from multihit_scenes import aimed_rays
    sd = scene_cache("atrium", detail=1)
    s = Scene(sd, device=gpu)
    n, k = 4096, 4
    pos = point_mix(sd, n, 81)
    org, dirs = aimed_rays(sd, n, 3)
    want_p, want_m = s.nearest_host(pos, k), s.multihit_host(org, dirs, k)
    st1, st2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    p, o, d = (torch.from_numpy(a).cuda() for a in (pos, org, dirs))
    d2 = torch.full((n, k), 5.0, dtype=torch.float32, device="cuda")
    ptri = torch.full((n, k), 5, dtype=torch.int32, device="cuda")
    pcnt = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    t = torch.full((n, k), 5.0, dtype=torch.float32, device="cuda")
    mtri = torch.full((n, k), 5, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        s.closest_points_multi_device(n, k, p.data_ptr(), d_dist2=d2.data_ptr(), d_tri=ptri.data_ptr(), d_count=pcnt.data_ptr(), stream=st1.cuda_stream)
        s.trace_multi_device(n, k, o.data_ptr(), d.data_ptr(), d_t=t.data_ptr(), d_tri=mtri.data_ptr(), d_count=cnt.data_ptr(), stream=st2.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d2.cpu().numpy().view(np.uint32), want_p["dist2"].view(np.uint32))
    np.testing.assert_array_equal(ptri.cpu().numpy().view(np.uint32), want_p["tri"])
    np.testing.assert_array_equal(pcnt.cpu().numpy().view(np.uint32), want_p["count"])
    np.testing.assert_array_equal(t.cpu().numpy(), want_m["t"])
    np.testing.assert_array_equal(mtri.cpu().numpy().view(np.uint32), want_m["tri"])
    np.testing.assert_array_equal(cnt.cpu().numpy().view(np.uint32), want_m["count"])
    s.close()


# ---- the empty scene and the single triangle ---------------------------------------------------------------------------------------------------
def test_the_empty_scene_and_the_single_triangle(gpu):
    g = np.random.default_rng(5)
    pos = g.uniform(-2.0, 2.0, (300, 3)).astype(f32)
    s = Scene(scenes.get_scene("empty"), device=gpu)
    for k in (1, 8):
        want = hold(s, pos, k, f"empty k={k}")
        assert (want["count"] == 0).all() and (want["tri"] == NO_TRI).all() and np.isinf(want["dist2"]).all()
    s.close()
    sd = scenes.get_scene("triangle")
    s = Scene(sd, device=gpu)
    pos = point_mix(sd, 300, 6)
    for k in (1, 2, 8):
        want = hold(s, pos, k, f"triangle k={k}")
        assert (want["count"] == 1).all() and (want["tri"][:, 0] == 0).all() and (want["tri"][:, 1:] == NO_TRI).all()
    key = (np.ascontiguousarray(want["dist2"][:, 0]), np.zeros(len(pos), np.uint32))
    assert (hold(s, pos, 2, "triangle behind its own key", None, key)["count"] == 0).all()
    s.close()


# ---- more entries than the persistent grid has lanes ----------------------------------------------------------------------------------------
def test_every_wave_of_the_product_grid_claims_again(gpu):
    """The Cornell box at n = 2^20 + 17 with k = 2: more points than the product's persistent grid has lanes (three workgroups of 512 per CU
    at the most), so every wave refills from the shards until they are exhausted. The points are the 2,048 of the small case, repeated:
    the expected value is the model, repeated."""
    import torch
    c = small_case("cornell")
    n = 2 ** 20 + 17
    assert n > 3 * 512 * torch.cuda.get_device_properties(0).multi_processor_count
    rep = -(-n // len(c["pos"]))
    pos = np.tile(c["pos"], (rep, 1))[:n]
    m = nearest_model(c["table"], 2)
    s = Scene(c["sd"], device=gpu)
    got = near_dev(s, pos, 2)
    for name in OUTPUTS:
        want = np.tile(m[name], (rep, 1) if m[name].ndim == 2 else rep)[:n]
        np.testing.assert_array_equal(got[name].view(np.uint32), want.view(np.uint32), err_msg=name)
    s.close()
