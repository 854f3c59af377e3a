"""Occlusion gathers on the device (rt_gather_occlusion[_device], k_occlusion_gather): the device form and the host form against
rt_scene_occlusion_host(use_bvh = 0) on the same scene object and against the numpy model over the device's own RT_QUERY_ANY ray queries
(tests/occlusion_scenes.py; tests/test_occlusion.py holds the host brute force to the oracle without a GPU). Every comparison is bit for
bit."""
import numpy as np
import pytest

import closest_scenes as cs
import occlusion_scenes as oc
from occlusion_scenes import OUTPUTS, device_occluder, mix_case, occlusion_model, same
from rtamd import abi, scenes
from rtamd.renderer import Scene
from test_path_query import scene_bounds

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    return 0


def occlusion_dev(s, pos, nrm, state, samples, max_dist=None, stream=None, outputs=OUTPUTS, canary=7, in_place=False):
    """rt_gather_occlusion_device on torch tensors; returns numpy results (outputs not asked for keep the canary). in_place: rng_out == rng"""
    import torch
    n = len(pos)
    up = lambda a, dt: torch.from_numpy(np.array(a, dt, order="C")).cuda()  # (a copy: the shared cases are read-only)
    p, nr = up(pos, f32), up(nrm, f32)
    st_in = up(np.asarray(state, np.uint32).view(np.int32), np.int32)
    md = up(max_dist, f32) if max_dist is not None else None
    st = stream or torch.cuda.current_stream()
    shape = {"bent": (n, 3)}
    bufs = {name: torch.full(shape.get(name, (n,)), canary, dtype=torch.float32 if name in ("visibility", "bent") else torch.int32, device="cuda")
            for name in OUTPUTS}
    if in_place:
        bufs["rng"] = st_in
    torch.cuda.synchronize()
    ptr = {"d_" + ("rng_out" if name == "rng" else name): bufs[name].data_ptr() for name in outputs}
    s.gather_occlusion_device(n, p.data_ptr(), nr.data_ptr(), st_in.data_ptr(), samples, d_max_dist=md.data_ptr() if md is not None else 0,
                              stream=st.cuda_stream, **ptr)
    st.synchronize()
    out = {name: bufs[name].cpu().numpy() for name in OUTPUTS}
    for name in ("clear", "rays", "rng"):
        out[name] = out[name].view(np.uint32)
    return out


def hold(s, pos, nrm, state, samples, what, max_dist=None, chain=True):
    """device form == host form == occlusion_host(use_bvh = 0) on the same scene == the model over the device's ANY queries"""
    want = s.occlusion_host(pos, nrm, state, samples, max_dist)
    same(occlusion_dev(s, pos, nrm, state, samples, max_dist), want, f"{what}: device")
    same(s.gather_occlusion(pos, nrm, state, samples, max_dist), want, f"{what}: host form")
    if chain:
        same(occlusion_model(device_occluder(s), pos, nrm, state, samples, max_dist), want, f"{what}: chain of ANY queries")
    return want


# ---- sizes and samples -----------------------------------------------------------------------------------------------------------------------
def test_cornell_at_every_size_with_and_without_restarts(gpu):
    """n = 1, 63, 64, 65 and 513 (one lane, a wave less one, a wave, a wave and one, a workgroup and one) and 2,000; samples = 1 (the
    restart path never taken), 2, 3 and 16; free and under the radius mix."""
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=gpu)
    pos, nrm, state, _ = oc.entries(sd, 2000, 41)
    radii = oc.radius_mix(2000, scene_bounds(sd)[2], 43)
    for n in (1, 63, 64, 65, 513, 2000):
        for samples in (1, 2, 3, 16):
            free = hold(s, pos[:n], nrm[:n], state[:n], samples, f"cornell n={n} samples={samples}", chain=n in (65, 2000))
            mix = hold(s, pos[:n], nrm[:n], state[:n], samples, f"cornell n={n} samples={samples} mix", radii[:n], chain=n in (65, 2000))
    assert 0 < free["clear"].sum() < mix["clear"].sum() < 16 * 2000
    s.close()


def test_the_mix_on_the_tables(gpu):
    """(the coarse atrium's expected side is a brute force over 235,750 triangles: tests/test_occlusion.py holds it on the CPU, and the atrium
    at detail 1 stands for it below)"""
    c = mix_case("tables")
    s = Scene(c["sd"], device=gpu)
    for samples in (1, 7):
        hold(s, c["pos"], c["nrm"], c["state"], samples, f"tables samples={samples}")
        hold(s, c["pos"], c["nrm"], c["state"], samples, f"tables samples={samples} mix", c["radii"])
    s.close()


# ---- refills, restarts and the drain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3])
def test_waves_refill_beside_busy_lanes(gpu, devlib, monkeypatch, grid):
    """5,000 entries of the Cornell box under RT_OCCLUSION_GRID = 1 and 3 (the developer build's knob, read at a scene's first occlusion
    launch): one or three workgroups claim the whole list, so every wave takes new entries beside lanes that are between two samples."""
    monkeypatch.setenv("RT_OCCLUSION_GRID", str(grid))
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=gpu, lib=devlib)
    pos, nrm, state, _ = oc.entries(sd, 5000, 17)
    radii = oc.radius_mix(5000, scene_bounds(sd)[2], 19)
    for samples in (1, 5):
        hold(s, pos, nrm, state, samples, f"grid {grid} samples={samples} mix", radii, chain=False)
    hold(s, pos, nrm, state, 3, f"grid {grid} free", chain=False)
    s.close()


def test_one_wave_whose_even_lanes_end_at_the_root(gpu, devlib, monkeypatch):
    """n = 64 under RT_OCCLUSION_GRID = 1, samples = 7: the even entries have max_dist = -1, so each of their traversals ends at the root
    and their restarts pile up beside the odd entries' unbounded walks; once the shards are exhausted the wave drains lanes that are done
    traversing but have samples left."""
    monkeypatch.setenv("RT_OCCLUSION_GRID", "1")
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=gpu, lib=devlib)
    g = np.random.default_rng(3)
    lo, hi, _ = scene_bounds(sd)
    pos = g.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (64, 3)).astype(f32)
    nrm = g.normal(size=(64, 3)).astype(f32)
    state = g.integers(1, 2**32, 64, dtype=np.uint64).astype(np.uint32)
    md = np.where(np.arange(64) % 2 == 0, f32(-1.0), f32(np.inf)).astype(f32)
    want = hold(s, pos, nrm, state, 7, "one wave", md)
    assert (want["clear"][0::2] == 7).all() and (want["rays"] == 7).all() and (want["clear"][1::2] < 7).any()
    hold(s, pos[:33], nrm[:33], state[:33], 7, "half a wave", md[:33])
    s.close()


def test_a_wave_of_degenerate_entries(gpu):
    """n = 64, every entry's normal 1e20: no lane ever traverses, and every entry is stored — rays = 0, visibility = 1, bent = 0, the state
    3 x samples draws on. Then the same entries in front of and between ordinary ones."""
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=gpu)
    pos, nrm, state, _ = oc.entries(sd, 256, 5)
    huge = nrm.copy()
    huge[:64] = oc.HUGE_NORMAL
    for samples in (1, 7):
        got = occlusion_dev(s, pos[:64], huge[:64], state[:64], samples)
        assert (got["rays"] == 0).all() and (got["clear"] == samples).all() and (got["visibility"] == 1).all() and not got["bent"].any()
        np.testing.assert_array_equal(got["rng"], oc.steps(state[:64], 3 * samples))
        same(got, s.occlusion_host(pos[:64], huge[:64], state[:64], samples), "all degenerate")
        huge2 = huge.copy()
        huge2[100:200:3] = -oc.HUGE_NORMAL
        hold(s, pos, huge2, state, samples, f"degenerate entries among others, samples={samples}")
    s.close()


# ---- trees ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh", "lbvh_gpu"])
def test_the_atrium_under_every_builder(gpu, devlib, builder):
    sd = scenes.get_scene("atrium", detail=1)
    s = Scene(sd, gpu, cs.BUILDERS[builder], lib=devlib)
    assert s.tree()["built_by"] == cs.BUILDERS[builder]
    pos, nrm, state, _ = oc.entries(sd, 1024, 19)
    radii = oc.radius_mix(1024, scene_bounds(sd)[2], 23)
    want = hold(s, pos, nrm, state, 5, f"atrium {builder}")
    assert 0 < want["clear"].sum() < 5 * 1024
    hold(s, pos, nrm, state, 5, f"atrium {builder} mix", radii)
    same(s.occlusion_host(pos, nrm, state, 5, radii, use_bvh=True), s.occlusion_host(pos, nrm, state, 5, radii), f"atrium {builder}: host walk")
    s.close()


def test_an_updated_scene_equals_a_fresh_build(gpu):
    from test_scene_update import update_sequence
    sd = scenes.get_scene("atrium", detail=1)
    s = Scene(sd, gpu, abi.RT_BVH_LBVH, updatable=True)
    pos, nrm, state, _ = oc.entries(sd, 1024, 23)
    before = occlusion_dev(s, pos, nrm, state, 4)
    for u in update_sequence(sd)[:2]:
        s.update(**u)
    fresh = Scene(s.desc, gpu, abi.RT_BVH_LBVH)
    want = hold(fresh, pos, nrm, state, 4, "fresh build")
    same(occlusion_dev(s, pos, nrm, state, 4), want, "updated scene")
    same(s.occlusion_host(pos, nrm, state, 4, use_bvh=True), want, "updated scene, host walk")
    assert not np.array_equal(before["clear"], want["clear"])
    s.close(), fresh.close()


@pytest.mark.parametrize("builder", ["sah", "lbvh_gpu"])
def test_the_mixed_scene_is_the_chain_of_any_queries(gpu, builder):
    """Slivers and degenerate triangles: the brute force need not equal a walk there (the limit every ray query shares, DESIGN.md §14 and
    §24); the identity with the device's own chain of RT_QUERY_ANY queries holds on every entry."""
    sd, _ = cs.mixed_scene()
    s = Scene(sd, gpu, cs.BUILDERS[builder])
    pos, nrm, state, _ = oc.entries(sd, 2048, 13)
    nrm[~np.isfinite(nrm).all(1)] = np.array([0.0, 0.0, 1.0], f32)  # (a point on a degenerate triangle has no face normal: such an entry is rejected)
    radii = oc.radius_mix(2048, scene_bounds(sd)[2], 15)
    for samples, md in ((1, None), (6, None), (6, radii)):
        want = occlusion_model(device_occluder(s), pos, nrm, state, samples, md)
        same(occlusion_dev(s, pos, nrm, state, samples, md), want, f"mixed {builder} samples={samples}: device")
        same(s.gather_occlusion(pos, nrm, state, samples, md), want, f"mixed {builder} samples={samples}: host form")
    assert 0 < want["clear"].sum() < 6 * 2048
    s.close()


# ---- rejected entries, NULL outputs, aliasing --------------------------------------------------------------------------------------------------
def test_rejected_entries_are_marked_and_the_rest_answered(gpu):
    """The device form marks exactly the entries the host form refuses one by one: a pos outside the contract range or not finite, a
    normal component that is not finite, a NaN max_dist — visibility and bent NaN, clear = rays = 0xFFFFFFFF, rng_out = rng."""
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=gpu)
    n, samples = 256, 3
    pos, nrm, state, _ = oc.entries(sd, n, 29)
    md = oc.radius_mix(n, scene_bounds(sd)[2], 31)
    _, _, limit = cs.contract_limits(sd)
    pos[20, 0] = np.nan
    pos[70, 2] = np.inf
    pos[131] = pos[131] + f32(3.0) * limit
    nrm[33, 1] = np.nan
    nrm[90, 0] = -np.inf
    md[150] = np.nan
    bad = np.zeros(n, bool)
    bad[[20, 33, 70, 90, 131, 150]] = True
    got = occlusion_dev(s, pos, nrm, state, samples, md)
    assert np.isnan(got["visibility"][bad]).all() and np.isnan(got["bent"][bad]).all()
    assert (got["clear"][bad] == 0xFFFFFFFF).all() and (got["rays"][bad] == 0xFFFFFFFF).all()
    np.testing.assert_array_equal(got["rng"][bad], state[bad])
    want = s.occlusion_host(pos[~bad], nrm[~bad], state[~bad], samples, md[~bad])
    same({name: a[~bad] for name, a in got.items()}, want, "accepted entries")
    same(s.gather_occlusion(pos[~bad], nrm[~bad], state[~bad], samples, md[~bad]), want, "accepted entries, host form")
    for i in np.flatnonzero(bad):  # the host form refuses each of them alone, naming it
        one = slice(i, i + 1)
        with pytest.raises(abi.RtError) as e:
            s.gather_occlusion(pos[one], nrm[one], state[one], samples, md[one])
        assert e.value.status == abi.RT_ERR_INVALID and "entry 0" in str(e.value), i
    with pytest.raises(abi.RtError) as e:  # ... and names the FIRST in a list
        s.gather_occlusion(pos, nrm, state, samples, md)
    assert "entry 20" in str(e.value)
    s.close()


def test_null_outputs_are_left_alone_and_rng_out_may_be_rng(gpu):
    c = mix_case("cornell")
    s = Scene(c["sd"], device=gpu)
    pos, nrm, state, md = c["pos"], c["nrm"], c["state"], c["radii"]
    want = s.occlusion_host(pos, nrm, state, 4, md)
    for outputs in (("visibility",), ("bent",), ("clear", "rng"), ("rays",), ("visibility", "bent", "clear", "rays")):
        got = occlusion_dev(s, pos, nrm, state, 4, md, outputs=outputs, canary=7)
        for name in OUTPUTS:
            if name in outputs:
                np.testing.assert_array_equal(got[name], want[name], err_msg=str(outputs))
            else:
                assert (got[name] == 7).all(), (outputs, name)
    same(occlusion_dev(s, pos, nrm, state, 4, md, in_place=True), want, "rng_out == rng")
    s.close()


def test_an_occlusion_gather_and_a_nearest_query_on_two_streams_without_host_synchronisation(gpu, scene_cache):
    """The two launches share the scene's cursors: the later waits for the earlier on the device. Nothing synchronises between the
    enqueues; one synchronisation at the end."""
    import torch
    from test_closest_points import point_mix
    sd = scene_cache("atrium", detail=1)
    s = Scene(sd, device=gpu)
    n, k, samples = 4096, 4, 3
    pts = point_mix(sd, n, 81)
    pos, nrm, state, _ = oc.entries(sd, n, 3)
    want_n, want_o = s.nearest_host(pts, k), s.occlusion_host(pos, nrm, state, samples, use_bvh=True)
    st1, st2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    q, p, nr = (torch.from_numpy(a).cuda() for a in (pts, pos, nrm))
    rng = torch.from_numpy(state.view(np.int32)).cuda()
    d2 = torch.full((n, k), 5.0, dtype=torch.float32, device="cuda")
    ntri = torch.full((n, k), 5, dtype=torch.int32, device="cuda")
    vis = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
    bent = torch.full((n, 3), 5.0, dtype=torch.float32, device="cuda")
    rng_out = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        s.closest_points_multi_device(n, k, q.data_ptr(), d_dist2=d2.data_ptr(), d_tri=ntri.data_ptr(), stream=st1.cuda_stream)
        s.gather_occlusion_device(n, p.data_ptr(), nr.data_ptr(), rng.data_ptr(), samples, d_visibility=vis.data_ptr(), d_bent=bent.data_ptr(),
                                  d_rng_out=rng_out.data_ptr(), stream=st2.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d2.cpu().numpy(), want_n["dist2"])
    np.testing.assert_array_equal(ntri.cpu().numpy().view(np.uint32), want_n["tri"])
    np.testing.assert_array_equal(vis.cpu().numpy(), want_o["visibility"])
    np.testing.assert_array_equal(bent.cpu().numpy(), want_o["bent"])
    np.testing.assert_array_equal(rng_out.cpu().numpy().view(np.uint32), want_o["rng"])
    s.close()


def test_the_baker_on_the_device(gpu):
    from rtamd import bake
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=gpu)
    vis, bent = bake.bake_vertex_ao(s, sd, 8, 0.5, 9, repeats=2)
    host = type("H", (), {"gather_occlusion": lambda self, *a: s.occlusion_host(*a)})()
    hv, hb = bake.bake_vertex_ao(host, sd, 8, 0.5, 9, repeats=2)
    np.testing.assert_array_equal(vis, hv)
    np.testing.assert_array_equal(bent, hb)
    s.close()


# ---- more entries than the persistent grid has lanes ----------------------------------------------------------------------------------------
def test_every_wave_of_the_product_grid_claims_again(gpu):
    """The Cornell box at n = 2^20 + 17 with samples = 1: more entries than the product's persistent grid has lanes (three workgroups of
    512 per CU at the most), so every wave refills from the shards until they are exhausted. The entries are 2,048, repeated: the expected
    value is the host brute force's, repeated."""
    import torch
    sd = scenes.get_scene("cornell")
    n = 2 ** 20 + 17
    assert n > 3 * 512 * torch.cuda.get_device_properties(0).multi_processor_count
    pos, nrm, state, _ = oc.entries(sd, 2048, 41)
    rep = -(-n // 2048)
    s = Scene(sd, device=gpu)
    want = s.occlusion_host(pos, nrm, state, 1)
    got = occlusion_dev(s, np.tile(pos, (rep, 1))[:n], np.tile(nrm, (rep, 1))[:n], np.tile(state, rep)[:n], 1)
    for name in OUTPUTS:
        np.testing.assert_array_equal(got[name], np.tile(want[name], (rep, 1) if want[name].ndim == 2 else rep)[:n], err_msg=name)
    s.close()
