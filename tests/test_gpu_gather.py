"""Gather queries on the GPU (include/rt_mi355x.h: rt_gather_paths[_device], k_path_gather in rt_path_gather.hip). A gather takes and returns
every entry's RNG state, so it is bit for bit a chain of path queries: per sample draw the diffuse bounce's unit vector from the state
(tests/test_gather.py: unit_vector_model, pinned there to the oracle's scatter), trace one path from (pos, normal + unit) with the state, add.
The expected values are that chain over the oracle's path query (gather_model), and once over the device's own path queries; all three
outputs are compared with assert_array_equal throughout."""
import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd.renderer import Scene
from test_gather import DEPTH, MIX_N, gather_model, mix_case, mix_expected, sky_mean, steps
from test_path_query import probe_case

pytestmark = pytest.mark.gpu
f32 = np.float32
NAMES = ["cornell", "atrium", "tables"]


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    yield 0
    for s in _SCENES.values():  # the scenes the module's tests share
        s.close()
    _SCENES.clear()


_SCENES = {}


def case_scene(name, gpu):
    """the device scene of mix_case(name), built once per module"""
    if name not in _SCENES:
        _SCENES[name] = Scene(mix_case(name)[0], device=gpu)
    return _SCENES[name]


def assert_result(got, want, what):
    for k in ("radiance", "rng", "rays"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def _device_call(s, pos, nrm, state, depth, samples=1, in_place=False, want_rng=True, want_rays=True, stream=None, rr_start=0):
    """rt_gather_paths_device on torch tensors -> (radiance, rng_out or the rng tensor after the call, rays, the rng tensor), numpy; outputs
    start as 7.0 / 0x55 bytes"""
    import torch
    n = len(pos)
    p, nr = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    st = torch.from_numpy(state.view(np.int32)).cuda()
    rad = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    st_out = st if in_place else torch.full((n,), 0x55555555, dtype=torch.int32, device="cuda")
    rays = torch.full((n,), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.gather_paths_device(n, p.data_ptr(), nr.data_ptr(), st.data_ptr(), rad.data_ptr(), depth, samples=samples, rr_start=rr_start,
                          d_rng_out=st_out.data_ptr() if want_rng else 0, d_rays=rays.data_ptr() if want_rays else 0,
                          stream=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return rad.cpu().numpy(), st_out.cpu().numpy().view(np.uint32), rays.cpu().numpy().view(np.uint32), st.cpu().numpy().view(np.uint32)


# ---- 1. against the oracle on the mix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr_start", [0, 2])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_the_point_mix_equals_the_oracle(gpu, name, samples, rr_start):
    s = case_scene(name, gpu)
    pos, nrm, state = mix_case(name)[2]
    assert_result(s.gather_paths(pos, nrm, state, DEPTH, samples=samples, rr_start=rr_start), mix_expected(name, DEPTH, samples, rr_start),
                  f"{name}, samples {samples}, rr_start {rr_start}")


def test_the_point_mix_equals_the_oracle_in_the_device_form(gpu):
    import torch
    s = case_scene("atrium", gpu)
    pos, nrm, state = mix_case("atrium")[2]
    rad, st_out, rays, st_in = _device_call(s, pos, nrm, state, DEPTH, samples=3, rr_start=2, stream=torch.cuda.Stream(device=0))
    assert_result({"radiance": rad, "rng": st_out, "rays": rays}, mix_expected("atrium", DEPTH, 3, 2), "device form")
    np.testing.assert_array_equal(st_in, state)  # rng_out elsewhere: the input states are read only


# ---- 2. against the device's own path queries: the identity, independent of the oracle ----------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "tables"])
def test_a_gather_is_a_chain_of_the_devices_path_queries(gpu, name):
    s = case_scene(name, gpu)
    pos, nrm, state = mix_case(name)[2]
    assert_result(s.gather_paths(pos, nrm, state, DEPTH, samples=3, rr_start=2), gather_model(s.trace_paths, pos, nrm, state, DEPTH, 3, 2), name)


# ---- 3. prefixes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 2047, 2049])
def test_prefixes_of_the_mix_around_the_shard_and_chunk_sizes(gpu, n):
    """The first n entries: shard k of the 32 holds entries [n k / 32, n (k + 1) / 32). Below 32 most shards are empty, at 32 each holds one
    entry, at 33 one holds two; 63, 64 and 65 lie around a wave and a chunk; 2047 and 2049 around 64 entries per shard. An entry's result
    depends on its own three inputs alone."""
    s = case_scene("atrium", gpu)
    pos, nrm, state = mix_case("atrium")[2]
    want = {k: v[:n] for k, v in mix_expected("atrium", DEPTH, 3, 2).items()}
    assert_result(s.gather_paths(pos[:n], nrm[:n], state[:n], DEPTH, samples=3, rr_start=2), want, f"n = {n}")


# ---- 4. samples ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr_start", [0, 2])
def test_four_samples_are_four_chained_single_sample_gathers(gpu, rr_start):
    s = case_scene("atrium", gpu)
    pos, nrm, state = mix_case("atrium")[2]
    one = s.gather_paths(pos, nrm, state, DEPTH, samples=4, rr_start=rr_start)
    total, rays, st = np.zeros_like(pos), np.zeros(len(pos), np.uint32), state
    for _ in range(4):
        out = s.gather_paths(pos, nrm, st, DEPTH, samples=1, rr_start=rr_start)
        total, rays, st = total + out["radiance"], rays + out["rays"], out["rng"]
    np.testing.assert_array_equal(one["radiance"], total / f32(4.0))  # ((r0 + r1) + r2) + r3 over 4.0f
    np.testing.assert_array_equal(one["rng"], st)
    np.testing.assert_array_equal(one["rays"], rays)
    assert rays.max() > 4 and (one["rng"] != state).any()


# ---- 5. a grid far smaller than the entry list: every wave refills mid-flight -------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3])
def test_a_grid_of_one_and_of_three_workgroups_gathers_the_whole_mix(gpu, devlib, monkeypatch, grid):
    """RT_GATHER_GRID (developer library only) caps the persistent grid. With one workgroup eight waves share the mix's 65 chunks: every
    wave takes new entries beside live ones many times, hands a claimed chunk out in parts over several rounds, reuses its lanes for entry
    after entry and walks all 32 shards. 3 does not divide 32: the workgroups start on shards 0, 1 and 2."""
    monkeypatch.setenv("RT_GATHER_GRID", str(grid))
    product = case_scene("atrium", gpu)
    small = Scene(mix_case("atrium")[0], device=gpu, lib=devlib)  # the knob is read at this scene's first gather query
    pos, nrm, state = mix_case("atrium")[2]
    assert len(pos) == MIX_N > 8 * grid * 64 * 2
    for rr_start in (0, 2):
        got = small.gather_paths(pos, nrm, state, DEPTH, samples=2, rr_start=rr_start)
        assert_result(got, mix_expected("atrium", DEPTH, 2, rr_start), f"grid {grid}, rr_start {rr_start}: oracle")
        assert_result(got, product.gather_paths(pos, nrm, state, DEPTH, samples=2, rr_start=rr_start), f"grid {grid}, rr_start {rr_start}: product")
    small.close()


# ---- 6. the size at which the product's own grid is the smaller ----------------------------------------------------------------------------------
FULL_N = (1 << 20) + 17


def test_an_entry_list_larger_than_the_persistent_grid(gpu):
    """2^20 + 17 entries: the mix's entries tiled in a shuffled order, so the expected value is the oracle's result of the mix, indexed.
    The grid is the resident workgroups, 3 per CU (the LDS figure tests/test_gather.py checks), of 512 lanes each: above that many entries
    the launch stops growing and the waves live on refills. Once through the host form, once through the device form with nine rejected
    entries spread over the list (pos not finite, pos out of range, a NaN normal): a rejected entry leaves its lane idle inside the refill
    loop."""
    import torch
    s = case_scene("atrium", gpu)
    assert FULL_N > torch.cuda.get_device_properties(gpu).multi_processor_count * 3 * 512
    pos, nrm, state = mix_case("atrium")[2]
    want = mix_expected("atrium", DEPTH, 1, 0)
    index = np.arange(FULL_N) % MIX_N
    np.random.default_rng(23).shuffle(index)
    assert len(np.unique(index[:MIX_N])) < MIX_N and len(np.unique(index)) == MIX_N  # shuffled, and every entry of the mix is there
    p, nr, st = pos[index], nrm[index], state[index]
    assert_result(s.gather_paths(p, nr, st, DEPTH), {k: v[index] for k, v in want.items()}, "host form")
    bad = np.array([0, 63, 64, 4097, 393216, 393217, 700001, FULL_N - 65, FULL_N - 1])
    p[bad[0::3]] = [np.nan, 0.0, 0.0]
    p[bad[1::3]] = [0.0, 1e30, 0.0]  # finite, far outside the contract range
    nr[bad[2::3]] = [0.0, np.nan, 1.0]
    nr[bad[8]] = [np.inf, 0.0, 0.0]
    rad, st_out, rays, _ = _device_call(s, p, nr, st, DEPTH)
    assert np.isnan(rad[bad]).all() and (rays[bad] == 0xFFFFFFFF).all()
    np.testing.assert_array_equal(st_out[bad], st[bad])  # no draw taken
    rest = np.ones(FULL_N, bool)
    rest[bad] = False
    assert_result({"radiance": rad[rest], "rng": st_out[rest], "rays": rays[rest]}, {k: v[index][rest] for k, v in want.items()}, "device form")


# ---- 7. edges -----------------------------------------------------------------------------------------------------------------------------------
def test_the_host_form_refuses_rejected_entries_names_the_first_and_writes_nothing(gpu, rtlib):
    import ctypes as C
    s = case_scene("cornell", gpu)
    pos, nrm, state = (a[:130].copy() for a in mix_case("cornell")[2])
    for where, (arr, value) in {77: (pos, [0.0, 1e30, 0.0]), 40: (nrm, [0.0, -np.inf, 0.0]), 5: (pos, [np.nan, 0.0, 0.0])}.items():
        arr[where] = value  # added back to front: the first rejected entry moves forward each time
        with pytest.raises(abi.RtError) as e:
            s.gather_paths(pos, nrm, state, DEPTH)
        assert e.value.status == abi.RT_ERR_INVALID and f"entry {where}:" in str(e.value)
    rad, st_out, rays = np.full((130, 3), 7.0, f32), np.full(130, 0x55555555, np.uint32), np.full(130, 0x55555555, np.uint32)
    q = abi.rt_gather_query(n=130, max_depth=DEPTH, samples=1, rr_start=0, pos=pos.ctypes.data, normal=nrm.ctypes.data, rng=state.ctypes.data,
                            rng_out=st_out.ctypes.data, radiance=rad.ctypes.data, rays=rays.ctypes.data)
    assert rtlib.rt_gather_paths(s.h, C.byref(q)) == abi.RT_ERR_INVALID
    assert (rad == 7.0).all() and (st_out == 0x55555555).all() and (rays == 0x55555555).all()


def test_no_entry_and_one_entry(gpu):
    s = case_scene("cornell", gpu)
    pos, nrm, state = mix_case("cornell")[2]
    out = s.gather_paths(pos[:0], nrm[:0], state[:0], DEPTH)
    assert out["radiance"].shape == (0, 3) and out["rng"].shape == (0,) and out["rays"].shape == (0,)
    s.gather_paths_device(0, 0, 0, 0, 0, DEPTH)  # n == 0: RT_OK whatever the pointers
    want = mix_expected("cornell", DEPTH, 3, 0)
    k = 777
    assert_result(s.gather_paths(pos[k:k + 1], nrm[k:k + 1], state[k:k + 1], DEPTH, samples=3), {key: v[k:k + 1] for key, v in want.items()}, "n = 1")


def test_depth_one(gpu):
    """One ray per path: the sky where it leaves the scene, an emitter's radiance where it hits one, nothing elsewhere; rays == samples"""
    s = case_scene("tables", gpu)
    _, osc, (pos, nrm, state) = mix_case("tables")
    want = gather_model(osc.trace_paths, pos, nrm, state, 1, 2, 2)
    assert (want["rays"] == 2).all() and (want["radiance"] != 0).any()
    assert_result(s.gather_paths(pos, nrm, state, 1, samples=2, rr_start=2), want, "depth 1")


def test_states_in_place_and_outputs_left_out(gpu):
    s = case_scene("cornell", gpu)
    pos, nrm, state = (a[:700] for a in mix_case("cornell")[2])
    want = {k: v[:700] for k, v in mix_expected("cornell", DEPTH, 3, 0).items()}
    rad, st_out, rays, _ = _device_call(s, pos, nrm, state, DEPTH, samples=3, in_place=True)  # rng_out == rng
    assert_result({"radiance": rad, "rng": st_out, "rays": rays}, want, "in place")
    rad, st_out, rays, st_in = _device_call(s, pos, nrm, state, DEPTH, samples=3, want_rng=False, want_rays=False)  # both NULL
    np.testing.assert_array_equal(rad, want["radiance"])
    assert (st_out == 0x55555555).all() and (rays == 0x55555555).all()
    np.testing.assert_array_equal(st_in, state)


def test_empty_scene_returns_the_sky_after_one_ray_per_path_and_three_draws(gpu):
    sd = scenes.get_scene("empty")
    s = Scene(sd, device=gpu)
    g = np.random.default_rng(2)
    n = 300
    pos, nrm = g.normal(size=(n, 3)).astype(f32), g.normal(size=(n, 3)).astype(f32)
    state = g.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    for samples in (1, 2, 3):
        out = s.gather_paths(pos, nrm, state, DEPTH, samples=samples)
        np.testing.assert_array_equal(out["radiance"], np.tile(sky_mean(sd.sky, samples), (n, 1)))
        np.testing.assert_array_equal(out["rng"], steps(state, 3 * samples))
        assert (out["rays"] == samples).all()
    s.close()


# ---- 8. streams and updates ---------------------------------------------------------------------------------------------------------------------
def test_update_waits_for_a_pending_gather(gpu):
    """A device-form gather on a non-null stream behind a long kernel, then rt_scene_update: the gather returns what the scene held before,
    and afterwards the scene renders and gathers as a fresh build of the moved scene."""
    import torch
    from rtamd.renderer import Camera, MegakernelRenderer
    from test_scene_update import spin_about_centre
    sd, _, (pos, nrm, state) = mix_case("atrium")
    s = Scene(sd, device=gpu, updatable=True)
    before = mix_expected("atrium", DEPTH, 1, 0)
    n = len(pos)
    st = torch.cuda.Stream(device=0)
    p, nr = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    a = torch.from_numpy(state.view(np.int32)).cuda()
    rad = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    rays = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)  # ~0.1 s of spinning in front of the gather
    s.gather_paths_device(n, p.data_ptr(), nr.data_ptr(), a.data_ptr(), rad.data_ptr(), DEPTH, d_rng_out=a.data_ptr(), d_rays=rays.data_ptr(),
                          stream=st.cuda_stream)
    s.update(instances=spin_about_centre(sd, 25.0))
    torch.cuda.synchronize()
    assert_result({"radiance": rad.cpu().numpy(), "rng": a.cpu().numpy().view(np.uint32), "rays": rays.cpu().numpy().view(np.uint32)}, before, "pending")
    fresh = Scene(s.desc, device=gpu)
    after, moved = s.gather_paths(pos, nrm, state, DEPTH), fresh.gather_paths(pos, nrm, state, DEPTH)
    assert not np.array_equal(moved["radiance"], before["radiance"])  # the update did move the scene
    assert_result(after, moved, "gather after the update")
    w, h = 64, 36
    cam = Camera.for_scene(sd, (w, h))
    frames = []
    for sc in (s, fresh):
        r = MegakernelRenderer(sc, (w, h), DEPTH, 2)
        frames.append(r.render_frame(cam))
        r.close()
    np.testing.assert_array_equal(frames[0].rgba_f32, frames[1].rgba_f32)
    assert frames[0].rays == frames[1].rays
    fresh.close(), s.close()


@pytest.mark.parametrize("other", ["path", "ray"])
def test_a_gather_and_another_query_back_to_back_on_two_streams(gpu, other):
    """They share the scene's ray cursors: the later launch waits for the earlier one on the device, and each returns what it returns alone.
    Both orders."""
    import torch
    s = case_scene("atrium", gpu)
    pos, nrm, state = mix_case("atrium")[2]
    n = len(pos)
    alone_g = mix_expected("atrium", DEPTH, 1, 0)
    org, d, state_p = probe_case("atrium")[2]  # the other query's own rays (tests/test_path_query.py: probe_mix), as many as the gather has entries
    assert len(org) == n
    alone_t = s.trace(org, d)
    alone_p = s.trace_paths(org, d, state_p, DEPTH)
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    p, nr = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    a = torch.from_numpy(state.view(np.int32)).cuda()
    o, di = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    b = torch.from_numpy(state_p.view(np.int32)).cuda()
    for gather_first in (False, True):
        t = torch.zeros(n, dtype=torch.float32, device="cuda")
        tri = torch.zeros(n, dtype=torch.int32, device="cuda")
        rad_p = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        a_p = torch.zeros(n, dtype=torch.int32, device="cuda")
        rad_g = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        a_g = torch.zeros(n, dtype=torch.int32, device="cuda")
        rays_g = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(50_000_000)
        if other == "ray":
            second = lambda st: s.trace_device(n, o.data_ptr(), di.data_ptr(), d_t=t.data_ptr(), d_tri=tri.data_ptr(), stream=st.cuda_stream)  # noqa: E731
        else:
            second = lambda st: s.trace_paths_device(n, o.data_ptr(), di.data_ptr(), b.data_ptr(), rad_p.data_ptr(), DEPTH,  # noqa: E731
                                                     d_rng_out=a_p.data_ptr(), stream=st.cuda_stream)
        calls = [second, lambda st: s.gather_paths_device(n, p.data_ptr(), nr.data_ptr(), a.data_ptr(), rad_g.data_ptr(), DEPTH,
                                                          d_rng_out=a_g.data_ptr(), d_rays=rays_g.data_ptr(), stream=st.cuda_stream)]
        if gather_first:
            calls.reverse()
        calls[0](sa), calls[1](sb)
        torch.cuda.synchronize()
        assert_result({"radiance": rad_g.cpu().numpy(), "rng": a_g.cpu().numpy().view(np.uint32), "rays": rays_g.cpu().numpy().view(np.uint32)},
                      alone_g, f"gather, gather_first {gather_first}")
        if other == "ray":
            np.testing.assert_array_equal(t.cpu().numpy(), alone_t[0])
            np.testing.assert_array_equal(tri.cpu().numpy().view(np.uint32), alone_t[3])
        else:
            np.testing.assert_array_equal(rad_p.cpu().numpy(), alone_p["radiance"])
            np.testing.assert_array_equal(a_p.cpu().numpy().view(np.uint32), alone_p["rng"])


# ---- 9. the baker -----------------------------------------------------------------------------------------------------------------------------------
def test_bake_vertices_is_the_mean_of_gathers_with_the_same_seeds(gpu):
    sd = mix_case("cornell")[0]
    s = case_scene("cornell", gpu)
    samples, seed = 3, 11
    got = bake.bake_vertices(s, sd, samples, DEPTH, seed, repeats=2)
    pos, nrm = bake.vertex_points(sd)
    c = sd.n_triangles * 3
    seeds = bake.corner_seeds(c, 2, seed)
    runs = [s.gather_paths(pos.reshape(c, 3), nrm.reshape(c, 3), seeds[:, k], DEPTH, samples=samples)["radiance"] for k in range(2)]
    assert got.shape == (sd.n_triangles, 3, 3) and got.dtype == f32
    np.testing.assert_array_equal(got.reshape(c, 3), (runs[0] + runs[1]) / f32(2.0))
    assert (got != 0).any()
