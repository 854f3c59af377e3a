"""Multi-hit ray queries on the device (rt_trace_rays_multi[_device], k_multihit<2 / 4 / 8>): the device form and the host form against
rt_scene_multihit_host(use_bvh = 0) on the same scene object and, on the three small scenes, against the oracle-table model
(tests/multihit_scenes.py; tests/test_multihit.py holds the host brute force to it without a GPU). Every comparison is bit for bit."""
import numpy as np
import pytest

import closest_scenes as cs
import multihit_scenes as ms
from multihit_scenes import OUTPUTS, aimed_rays, multihit_model, same, small_case
from rtamd import abi, scenes
from rtamd.renderer import Scene
from test_closest_points import NO_TRI
from test_multihit import key_mix

pytestmark = pytest.mark.gpu
f32 = np.float32
SLOTS = ("t", "u", "v", "tri")


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    return 0


def multi_dev(s, org, dirs, k, tmax=None, after=None, stream=None, outputs=OUTPUTS, canary=7):
    """rt_trace_rays_multi_device on torch tensors; returns numpy results (outputs not asked for keep the canary)"""
    import torch
    n = len(org)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    o, d = up(org, f32), up(dirs, f32)
    tm = up(tmax, f32) if tmax is not None else None
    at, atri = (up(after[0], f32), up(np.asarray(after[1], np.uint32).view(np.int32), np.int32)) if after is not None else (None, None)
    st = stream or torch.cuda.current_stream()
    bufs = {name: torch.full((n,) if name == "count" else (n, k), canary, dtype=torch.int32 if name in ("tri", "count") else torch.float32, device="cuda")
            for name in OUTPUTS}
    torch.cuda.synchronize()
    s.trace_multi_device(n, k, o.data_ptr(), d.data_ptr(), d_tmax=tm.data_ptr() if tm is not None else 0,
                         d_after_t=at.data_ptr() if at is not None else 0, d_after_tri=atri.data_ptr() if atri is not None else 0,
                         stream=st.cuda_stream, **{"d_" + name: bufs[name].data_ptr() for name in outputs})
    st.synchronize()
    out = {name: bufs[name].cpu().numpy() for name in OUTPUTS}
    out["tri"], out["count"] = out["tri"].view(np.uint32), out["count"].view(np.uint32)
    return out


def hold(s, org, dirs, k, what, tmax=None, after=None, model=None):
    """device form == host form == multihit_host(use_bvh = 0) on the same scene (== `model` where given) -> the brute force's result"""
    want = s.multihit_host(org, dirs, k, tmax, after)
    if model is not None:
        same(want, model, f"{what}: brute force vs model")
    same(multi_dev(s, org, dirs, k, tmax, after), want, f"{what}: device")
    same(s.trace_multi(org, dirs, k, tmax, after), want, f"{what}: host form")
    return want


# ---- the three small scenes, against the oracle's table -------------------------------------------------------------------------------------
def test_cornell_equals_the_model_at_every_size(gpu):
    """n = 1, 63, 64, 65 and 513 (one lane, a wave less one, a wave, a wave and one, a workgroup and one) and 2,000; k = 1, 2 and 8 (the
    three instantiations), free and under the tmax and key mix."""
    c = small_case("cornell")
    s = Scene(c["sd"], device=gpu)
    free = multihit_model(c["table"], 8)
    tmax, after = key_mix(free, 3)
    for n in (1, 63, 64, 65, 513, 2000):
        tab = {name: a[:, :n] for name, a in c["table"].items()}
        org, d = c["org"][:n], c["dirs"][:n]
        for k in (1, 2, 8):
            hold(s, org, d, k, f"cornell n={n} k={k}", model=multihit_model(tab, k))
        mix = (tmax[:n], (after[0][:n], after[1][:n]))
        hold(s, org, d, 4, f"cornell n={n} k=4 mix", *mix, model=multihit_model(tab, 4, *mix))
    s.close()


@pytest.mark.parametrize("k", range(1, 9))
def test_ties_across_the_last_slot_on_the_duplicates(gpu, k):
    """Seven shuffled cubes: every hit is a seven-fold tie, and in one of the two runs of every k (multihit_scenes.duplicate_runs) the tie
    straddles slot k - 1 on every ray — the entry that stays is the one with the lower index, the box at the bound's distance is kept."""
    c = small_case("duplicates")
    s = Scene(c["sd"], device=gpu)
    for what, after in ms.duplicate_runs(c["table"], k):
        hold(s, c["org"], c["dirs"], k, f"duplicates k={k} {what}", None, after, model=multihit_model(c["table"], k, None, after))
    s.close()


def test_every_instantiation_is_reached_and_the_wrong_one_would_fail(gpu):
    """The pile of 256: k = 3 on rays with at least 4 hits (a 2-slot list could not hold them, a bound on the wrong slot would keep the
    fourth), k = 5 .. 8 on rays with at least 9 (a 4-slot list could not), and k = 2 / 4 / 8 at the top of each list."""
    c = small_case("pile256")
    hits = ms.hits_per_ray(c["table"])
    assert (hits >= 9).mean() >= 0.5
    s = Scene(c["sd"], device=gpu)
    for k in (2, 3, 4, 5, 7, 8):
        want = hold(s, c["org"], c["dirs"], k, f"pile256 k={k}", model=multihit_model(c["table"], k))
        assert ((want["count"] == k) & (hits > k)).mean() >= 0.5  # at least half of the lists are full with more hits behind them
    s.close()


# ---- refills beside live lanes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3])
def test_waves_refill_beside_live_lanes(gpu, devlib, monkeypatch, grid):
    """5,000 aimed rays of the Cornell box under RT_MULTIHIT_GRID = 1 and 3 (the developer build's knob, read at a scene's first multi-hit
    launch): one or three workgroups claim the whole list, so every wave opens new lists beside lanes that hold full ones; with the tmax
    and key mix a quarter of the rays end at the root."""
    monkeypatch.setenv("RT_MULTIHIT_GRID", str(grid))
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=gpu, lib=devlib)
    org, d = aimed_rays(sd, 5000, 17)
    free = hold(s, org, d, 8, f"grid {grid}")
    tmax, after = key_mix(free, 5)
    for k in (2, 3, 8):
        hold(s, org, d, k, f"grid {grid} k={k} mix", tmax, after)
    s.close()


# ---- deep stacks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh", "lbvh_gpu"])
def test_the_full_pile_spills_the_stack_under_a_moving_bound(gpu, devlib, monkeypatch, builder):
    """8,192 parallel triangles in one box: stack_need > kLdsStack on the very tree the kernel walks, so lanes push and pop through the
    spill routines while their bound moves. k = 8 and k = 3 on 1,024 aimed rays. Then one wave (n = 64 under RT_MULTIHIT_GRID=1) whose even
    rays have tmax = -1 — the root is visited, nothing is entered, the sentinel is popped — and whose odd rays are unbounded."""
    sd = cs.pile_scene()
    s = Scene(sd, gpu, cs.BUILDERS[builder], lib=devlib)
    tree = s.tree()
    assert tree["stack_need"] > cs.K_LDS_STACK and tree["built_by"] == cs.BUILDERS[builder]
    org, d = aimed_rays(sd, 1024, 7)
    want = hold(s, org, d, 8, f"pile {builder} k=8")
    assert (want["count"] == 8).mean() > 0.4
    hold(s, org, d, 3, f"pile {builder} k=3")
    s.close()
    monkeypatch.setenv("RT_MULTIHIT_GRID", "1")
    s = Scene(sd, gpu, cs.BUILDERS[builder], lib=devlib)
    assert s.tree()["stack_need"] > cs.K_LDS_STACK
    tmax = np.where(np.arange(64) % 2 == 0, f32(-1.0), f32(np.inf)).astype(f32)
    want = s.multihit_host(org[:64], d[:64], 8, tmax)
    assert (want["count"][0::2] == 0).all() and (want["count"][1::2] > 0).any()
    same(multi_dev(s, org[:64], d[:64], 8, tmax), want, f"pile {builder}: one wave, shallow and spilled lanes")
    s.close()


# ---- de-duplication and NaN candidates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh", "lbvh_gpu"])
def test_the_mixed_scene_lists_pre_split_triangles_once(gpu, builder):
    """Two scene-spanning triangles (pre-split under SAH: whole in many leaves) over 3,000 tiny ones, 500 slivers and 300 degenerate
    triangles whose candidates are NaN or never exist, against the host brute force over the triangle list. 2,048 rays through triangle
    centroids, ALL of them held to the contract with its stated limit (multihit_scenes.held_to_the_limit): the device form's and the host
    form's list is the brute force's with nothing but ill-conditioned hits dropped — hits on slivers whose fp32 t is more than half the
    boxes' padding from their true t, which a tree may cull behind the bound or tmax, for every ray query of the library (DESIGN.md
    §24). On the 1,822 rays without such a hit that is the brute force's list itself, asserted on its own as well."""
    sd, _ = cs.mixed_scene()
    s = Scene(sd, gpu, cs.BUILDERS[builder])
    assert (s.info().n_split_triangles > 0) == (builder == "sah")
    org, d = ms.rays_at_triangles(sd, 2048, 13)
    ok = ms.well_conditioned(s, org, d)
    assert ok.sum() == 1822
    want = s.multihit_host(org, d, 8)
    srt = np.sort(want["tri"], 1)
    assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != NO_TRI)).any() and (want["count"] >= 2).mean() > 0.5
    tmax, after = key_mix(want, 9)
    for k, tm, key in ((8, None, None), (1, None, None), (2, tmax, after), (4, tmax, after)):
        brute = s.multihit_host(org, d, k, tm, key)
        for form, got in (("device", multi_dev(s, org, d, k, tm, key)), ("host form", s.trace_multi(org, d, k, tm, key))):
            what = f"mixed {builder} k={k}{' mix' if tm is not None else ''}: {form}"
            same({name: got[name][ok] for name in OUTPUTS}, {name: brute[name][ok] for name in OUTPUTS}, what)
            lost = ms.held_to_the_limit(got, s, org, d, k, tm, key, what)
            # (printed, not pinned: the pinned figures are the host walk's, tests/test_multihit.py: MIXED_SAH_LOST)
            print(f"{what}: (rays whose list differs from the brute force's, hits dropped) {lost}")
    # the k = 1 identity holds on every ray, the ill-conditioned ones too: rt_trace_rays CLOSEST skips the same boxes
    got = s.trace_multi(org, d, 1)
    for name, w in zip(SLOTS, s.trace(org, d)):
        np.testing.assert_array_equal(got[name][:, 0], w, err_msg=f"mixed {builder}, k = 1 against CLOSEST: {name}")
    s.close()


# ---- real trees -------------------------------------------------------------------------------------------------------------------------------
TREES = {
    "atrium_sah": lambda gpu: Scene(scenes.get_scene("atrium", detail=1), gpu, abi.RT_BVH_SAH),
    "atrium_lbvh_gpu": lambda gpu: Scene(scenes.get_scene("atrium", detail=1), gpu, abi.RT_BVH_LBVH_GPU),
    "tilted_sah": lambda gpu: Scene(scenes.atrium_tilted_scene(1), gpu, abi.RT_BVH_SAH),
}


@pytest.mark.parametrize("case", sorted(TREES))
def test_the_atrium(gpu, case):
    s = TREES[case](gpu)
    org, d = aimed_rays(s.desc, 1024, 19)
    want = hold(s, org, d, 8, f"{case} k=8")
    assert (want["count"] >= 2).mean() > 0.5
    tmax, after = key_mix(want, 4)
    hold(s, org, d, 4, f"{case} k=4 mix", tmax, after)
    hold(s, org, d, 1, f"{case} k=1")
    t, u, v, tri = s.trace(org, d)
    got = s.trace_multi(org, d, 1)
    for name, w in zip(SLOTS, (t, u, v, tri)):  # the k = 1 identity on the device: rt_trace_rays CLOSEST bit for bit
        np.testing.assert_array_equal(got[name][:, 0], w, err_msg=name)
    s.close()


def test_an_updated_scene_equals_a_fresh_build(gpu):
    from test_scene_update import update_sequence
    sd = scenes.get_scene("atrium", detail=1)
    s = Scene(sd, gpu, abi.RT_BVH_LBVH, updatable=True)
    org, d = aimed_rays(sd, 1024, 23)
    before = multi_dev(s, org, d, 8)
    for u in update_sequence(sd)[:2]:
        s.update(**u)
    fresh = Scene(s.desc, gpu, abi.RT_BVH_LBVH)
    want = hold(fresh, org, d, 8, "fresh build")
    same(multi_dev(s, org, d, 8), want, "updated scene")
    same(s.multihit_host(org, d, 8, use_bvh=True), want, "updated scene, host walk")
    assert not np.array_equal(before["t"], want["t"])
    s.close(), fresh.close()


# ---- paging on the device -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "pile256"])
def test_pages_of_two_fed_back_on_the_device_equal_one_call_of_eight(gpu, name):
    """Four pages of 2, each continued from the DEVICE buffers of the one before — the key is the page's last slot, gathered by a device
    copy on the same stream, no host round trip and no synchronisation between the pages. An exhausted ray's last slot is the miss,
    (+inf, 0xFFFFFFFF), a key behind which nothing counts: its later pages stay misses."""
    import torch
    c = small_case(name)
    s = Scene(c["sd"], device=gpu)
    n = len(c["org"])
    o, d = torch.from_numpy(c["org"]).cuda(), torch.from_numpy(c["dirs"]).cuda()
    st = torch.cuda.Stream(device=0)
    pages = [{k: torch.full((n, 2), 7, dtype=torch.int32 if k == "tri" else torch.float32, device="cuda") for k in SLOTS} for _ in range(4)]
    counts = [torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        at = atri = None
        for p, cnt in zip(pages, counts):
            s.trace_multi_device(n, 2, o.data_ptr(), d.data_ptr(), d_after_t=at.data_ptr() if at is not None else 0,
                                 d_after_tri=atri.data_ptr() if atri is not None else 0, d_count=cnt.data_ptr(), stream=st.cuda_stream,
                                 **{"d_" + k: p[k].data_ptr() for k in SLOTS})
            at, atri = p["t"][:, 1].contiguous(), p["tri"][:, 1].contiguous()
    st.synchronize()
    got = {k: np.concatenate([p[k].cpu().numpy() for p in pages], 1) for k in SLOTS}
    got["tri"] = got["tri"].view(np.uint32)
    got["count"] = sum(cnt.cpu().numpy().view(np.uint32) for cnt in counts)
    want = multihit_model(c["table"], 8)
    same(got, want, f"{name} pages of 2 on the device")
    same(got, s.multihit_host(c["org"], c["dirs"], 8), f"{name} pages of 2 vs the brute force")
    s.close()


# ---- rejected rays, NULL outputs ------------------------------------------------------------------------------------------------------------------
def test_rejected_rays_are_marked_and_the_rest_answered(gpu):
    """The device form marks exactly the rays the host form refuses one by one: an origin outside the contract range, a non-finite origin,
    a NaN tmax, a NaN after_t — every slot t = NaN and tri = RT_TRI_REJECTED, u and v unwritten, count = 0."""
    c = small_case("cornell")
    s = Scene(c["sd"], device=gpu)
    n, k = 256, 3
    org, d = c["org"][:n].copy(), c["dirs"][:n].copy()
    free = multihit_model({name: a[:, :n] for name, a in c["table"].items()}, 8)
    tmax, after = key_mix(free, 6)
    at, atri = after[0].copy(), after[1].copy()
    _, _, limit = cs.contract_limits(c["sd"])
    org[5, 0] = np.nan
    org[70, 2] = np.inf
    org[131] = org[131] + f32(3.0) * limit
    tmax[9] = np.nan
    at[200] = np.nan
    bad = np.zeros(n, bool)
    bad[[5, 9, 70, 131, 200]] = True
    got = multi_dev(s, org, d, k, tmax, (at, atri), canary=7)
    assert np.isnan(got["t"][bad]).all() and (got["tri"][bad] == abi.RT_TRI_REJECTED).all() and (got["count"][bad] == 0).all()
    assert (got["u"][bad] == 7).all() and (got["v"][bad] == 7).all()
    want = s.multihit_host(org[~bad], d[~bad], k, tmax[~bad], (at[~bad], atri[~bad]))
    same({name: a[~bad] for name, a in got.items()}, want, "accepted rays")
    same(s.trace_multi(org[~bad], d[~bad], k, tmax[~bad], (at[~bad], atri[~bad])), want, "accepted rays, host form")
    for i in np.flatnonzero(bad):  # the host form refuses each of them alone, naming it, and writes nothing
        one = slice(i, i + 1)
        with pytest.raises(abi.RtError) as e:
            s.trace_multi(org[one], d[one], k, tmax[one], (at[one], atri[one]))
        assert e.value.status == abi.RT_ERR_INVALID and "ray 0" in str(e.value), i
    keep = np.flatnonzero(~bad)[:4]
    for i in keep:
        one = slice(i, i + 1)
        s.trace_multi(org[one], d[one], k, tmax[one], (at[one], atri[one]))
    s.close()


def test_null_outputs_are_left_alone(gpu):
    c = small_case("cornell")
    s = Scene(c["sd"], device=gpu)
    want = multihit_model(c["table"], 4)
    for outputs in (("t",), ("tri", "count"), ("count",), ("u", "v")):
        got = multi_dev(s, c["org"], c["dirs"], 4, outputs=outputs, canary=7)
        for name in OUTPUTS:
            if name in outputs:
                np.testing.assert_array_equal(got[name], want[name], err_msg=str(outputs))
            else:
                assert (got[name] == 7).all(), (outputs, name)
    s.close()


def test_a_multihit_query_and_a_point_query_on_two_streams_without_host_synchronisation(gpu, scene_cache):
    """The two launches share the scene's cursors: the later waits for the earlier on the device. Nothing synchronises between the
    enqueues; one synchronisation at the end."""
    import torch
    from test_closest_points import point_mix
    sd = scene_cache("atrium", detail=1)
    s = Scene(sd, device=gpu)
    n, k = 4096, 4
    pos = point_mix(sd, n, 81)
    org, dirs = aimed_rays(sd, n, 3)
    want_p, want_m = s.closest_host(pos), s.multihit_host(org, dirs, k)
    st1, st2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    p, o, d = (torch.from_numpy(a).cuda() for a in (pos, org, dirs))
    d2 = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
    ptri = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    t = torch.full((n, k), 5.0, dtype=torch.float32, device="cuda")
    mtri = torch.full((n, k), 5, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        s.closest_points_device(n, p.data_ptr(), d_dist2=d2.data_ptr(), d_tri=ptri.data_ptr(), stream=st1.cuda_stream)
        s.trace_multi_device(n, k, o.data_ptr(), d.data_ptr(), d_t=t.data_ptr(), d_tri=mtri.data_ptr(), d_count=cnt.data_ptr(), stream=st2.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d2.cpu().numpy().view(np.uint32), want_p["dist2"].view(np.uint32))
    np.testing.assert_array_equal(ptri.cpu().numpy().view(np.uint32), want_p["tri"])
    np.testing.assert_array_equal(t.cpu().numpy(), want_m["t"])
    np.testing.assert_array_equal(mtri.cpu().numpy().view(np.uint32), want_m["tri"])
    np.testing.assert_array_equal(cnt.cpu().numpy().view(np.uint32), want_m["count"])
    s.close()


# ---- more entries than the persistent grid has lanes ----------------------------------------------------------------------------------------
def test_every_wave_of_the_product_grid_claims_again(gpu):
    """The Cornell box at n = 2^20 + 17 with k = 2: more rays than the product's persistent grid has lanes (three workgroups of 512 per CU at
    the most), so every wave refills from the shards until they are exhausted. The rays are the 2,048 of the small case, repeated: the
    expected value is the oracle-table model, repeated."""
    import torch
    c = small_case("cornell")
    n = 2 ** 20 + 17
    assert n > 3 * 512 * torch.cuda.get_device_properties(0).multi_processor_count
    rep = -(-n // len(c["org"]))
    org, d = np.tile(c["org"], (rep, 1))[:n], np.tile(c["dirs"], (rep, 1))[:n]
    m = multihit_model(c["table"], 2)
    s = Scene(c["sd"], device=gpu)
    got = multi_dev(s, org, d, 2)
    for name in OUTPUTS:
        want = np.tile(m[name], (rep, 1) if m[name].ndim == 2 else rep)[:n]
        np.testing.assert_array_equal(got[name], want, err_msg=name)
    s.close()
