"""Path queries on the GPU (include/rt_mi355x.h: rt_trace_paths[_device], k_path_query in rt_path_query.hip). The kernel runs the
renderers' own bounce on caller-supplied rays and returns every ray's RNG state, so a frame of the renderers is a chain of path queries:
seed every pixel as the renderer does, and per sample draw the camera ray (tests/test_path_query.py: get_ray_model), trace samples = 1 with
the running states and add the radiance. The renderers are pinned to the oracle bit for bit, and the queries are pinned to the renderers
here, with assert_array_equal throughout."""
import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer
from test_path_query import PROBE_N, get_ray_model, pixel_seed_model, probe_case, probe_expected

pytestmark = pytest.mark.gpu
f32 = np.float32

CASES = {  # name -> (scene, keywords, width, height)
    "cornell": ("cornell", {}, 48, 32),
    "atrium": ("atrium", {"coarse": True}, 64, 36),  # n = 2304: 72 rays per shard, a full chunk and a partial one; the height is no multiple of 8
    "tables": ("tables", {}, 48, 32),
}
DEPTH, SPP = 5, 3


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    yield 0
    for _, s in _SCENES.values():  # the scenes the module's tests share
        s.close()
    _SCENES.clear()


_SCENES = {}


def case_scene(name, gpu):
    """(description, device scene), built once per module"""
    if name not in _SCENES:
        sname, kw, _, _ = CASES[name]
        sd = scenes.table_scene() if sname == "tables" else scenes.get_scene(sname, **kw)
        _SCENES[name] = (sd, Scene(sd, device=gpu))
    return _SCENES[name]


def pixels(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return xs.ravel(), ys.ravel()


def camera_rays(cam, w, h, state):
    """(org, dir, state') of one sample of every pixel, row-major"""
    x, y = pixels(w, h)
    d, state = get_ray_model(cam.c, x, y, state)
    org = np.tile(np.array(list(cam.c.center), f32), (w * h, 1))
    return org, d, state


def chain(scene, cam, w, h, depth, spp, megakernel, salt=0, rr_start=0, clamp=False):
    """the frame as a chain of path queries: (fp32 frame (h, w, 4), unorm8 image, rays)"""
    x, y = pixels(w, h)
    state = pixel_seed_model(x, y, w, h, megakernel, salt)
    total = np.zeros((w * h, 3), f32)
    rays = 0
    for _ in range(spp):
        org, d, state = camera_rays(cam, w, h, state)
        out = scene.trace_paths(org, d, state, depth, samples=1, rr_start=rr_start)
        rad, state = out["radiance"], out["rng"]
        if clamp:  # clamp01 on every sample, as the wavefront renderer stores it (oracle_rt.cpp:843-848)
            rad = np.fmin(np.fmax(rad, f32(0)), f32(1))
        total = total + rad
        rays += int(out["rays"].astype(np.uint64).sum())
    c = np.sqrt(total / f32(spp))
    frame = np.concatenate([c, np.ones((w * h, 1), f32)], 1).reshape(h, w, 4)
    u8 = np.rint(np.fmin(np.fmax(c, f32(0)), f32(1)) * f32(255)).astype(np.uint8)
    image = np.concatenate([u8, np.full((w * h, 1), 255, np.uint8)], 1).reshape(h, w, 4)
    return frame, image, rays


def render(cls, scene, cam, w, h, depth, spp, salt=0, rr_start=0):
    r = cls(scene, (w, h), depth, spp)
    if salt:
        r.set_frame_seed(salt)
    if rr_start:
        r.set_russian_roulette(rr_start)
    fr = r.render_frame(cam)
    r.close()
    return fr


def assert_frame(got, fr, what):
    frame, image, rays = got
    np.testing.assert_array_equal(frame, fr.rgba_f32, err_msg=f"{what}: fp32 frame")
    np.testing.assert_array_equal(image, fr.rgba_u8, err_msg=f"{what}: unorm8 image")
    assert rays == fr.rays, what


# ---- 1. a frame is a chain of path queries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_megakernel_frame_is_a_chain_of_path_queries(gpu, name):
    sd, s = case_scene(name, gpu)
    _, _, w, h = CASES[name]
    cam = Camera.for_scene(sd, (w, h))
    fr = render(MegakernelRenderer, s, cam, w, h, DEPTH, SPP)
    assert fr.rgba_f32[..., :3].max() > 0 and fr.rays > w * h * SPP  # the frame shows something and paths do bounce
    assert_frame(chain(s, cam, w, h, DEPTH, SPP, megakernel=True), fr, name)


@pytest.mark.parametrize("name", list(CASES))
def test_a_wavefront_frame_is_the_chain_with_every_sample_clamped(gpu, name):
    sd, s = case_scene(name, gpu)
    _, _, w, h = CASES[name]
    cam = Camera.for_scene(sd, (w, h))
    fr = render(WavefrontRenderer, s, cam, w, h, DEPTH, SPP)
    assert_frame(chain(s, cam, w, h, DEPTH, SPP, megakernel=False, clamp=True), fr, name)


def test_the_chain_follows_the_frame_seed(gpu):
    sd, s = case_scene("atrium", gpu)
    _, _, w, h = CASES["atrium"]
    cam = Camera.for_scene(sd, (w, h))
    fr = render(MegakernelRenderer, s, cam, w, h, DEPTH, SPP, salt=5)
    got = chain(s, cam, w, h, DEPTH, SPP, megakernel=True, salt=5)
    assert_frame(got, fr, "salt 5")
    assert not np.array_equal(got[0], render(MegakernelRenderer, s, cam, w, h, DEPTH, SPP).rgba_f32)


# ---- 2. Russian roulette -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [MegakernelRenderer, WavefrontRenderer])
def test_russian_roulette(gpu, cls):
    sd, s = case_scene("cornell", gpu)
    _, _, w, h = CASES["cornell"]
    cam = Camera.for_scene(sd, (w, h))
    mega = cls is MegakernelRenderer
    fr = render(cls, s, cam, w, h, 8, SPP, rr_start=3)
    assert_frame(chain(s, cam, w, h, 8, SPP, megakernel=mega, rr_start=3, clamp=not mega), fr, "rr_start 3")
    assert fr.rays != render(cls, s, cam, w, h, 8, SPP).rays  # the roulette does end paths here


# ---- 3. samples ---------------------------------------------------------------------------------------------------------------------------------
def first_rays(name, gpu, cam=None):
    sd, s = case_scene(name, gpu)
    _, _, w, h = CASES[name]
    cam = cam or Camera.for_scene(sd, (w, h))
    x, y = pixels(w, h)
    return s, camera_rays(cam, w, h, pixel_seed_model(x, y, w, h, True))


@pytest.mark.parametrize("rr_start", [0, 2])
def test_samples_is_a_chain_of_single_paths_on_the_same_rays(gpu, rr_start):
    s, (org, d, state) = first_rays("atrium", gpu)
    one = s.trace_paths(org, d, state, DEPTH, samples=4, rr_start=rr_start)
    total, rays, st = np.zeros_like(org), np.zeros(len(org), np.uint32), state
    for _ in range(4):
        out = s.trace_paths(org, d, st, DEPTH, samples=1, rr_start=rr_start)
        total, rays, st = total + out["radiance"], rays + out["rays"], out["rng"]
    np.testing.assert_array_equal(one["radiance"], total / f32(4.0))  # ((r0 + r1) + r2) + r3 over 4.0f
    np.testing.assert_array_equal(one["rng"], st)
    np.testing.assert_array_equal(one["rays"], rays)
    assert rays.max() > 4 and (one["rng"] != state).any()


# ---- 4. a ray's result is its own ---------------------------------------------------------------------------------------------------------------
def test_a_rays_result_does_not_depend_on_its_batch(gpu):
    """The atrium's primary rays and those of two further cameras elsewhere in the hall, each traced in its camera's own call, then all of
    them shuffled and traced in batches of 1, 63, 64, 65 and the rest: every entry is what it was."""
    sd, s = case_scene("atrium", gpu)
    _, _, w, h = CASES["atrium"]
    p, dr = np.array(sd.camera.position, np.float64), np.array(sd.camera.direction, np.float64)
    side = np.cross(dr, [0.0, 1.0, 0.0])
    cams = [Camera.for_scene(sd, (w, h)), Camera((w, h), p + 0.35 * dr + 0.2 * side, dr - 0.8 * side, sd.camera.focal_length),
            Camera((w, h), p + 0.15 * dr - 0.3 * side + [0.0, 0.2, 0.0], -dr + 0.5 * side, sd.camera.focal_length)]
    orgs, dirs, states, own = [], [], [], []
    for cam in cams:
        _, (org, d, state) = first_rays("atrium", gpu, cam)
        orgs.append(org), dirs.append(d), states.append(state)
        own.append(s.trace_paths(org, d, state, DEPTH, samples=2))
    org, d, state = np.concatenate(orgs), np.concatenate(dirs), np.concatenate(states)
    want = {k: np.concatenate([o[k] for o in own]) for k in ("radiance", "rng", "rays")}
    assert len({tuple(o) for o in org}) == 3  # mixed origins
    perm = np.random.default_rng(11).permutation(len(org))
    org, d, state = org[perm], d[perm], state[perm]
    got = {k: [] for k in want}
    at = 0
    for size in (1, 63, 64, 65, len(org) - 193):
        out = s.trace_paths(org[at:at + size], d[at:at + size], state[at:at + size], DEPTH, samples=2)
        for k in got:
            got[k].append(out[k])
        at += size
    assert at == len(org)
    for k in want:
        np.testing.assert_array_equal(np.concatenate(got[k]), want[k][perm], err_msg=k)


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------------------
def test_no_ray_and_one_ray(gpu):
    s, (org, d, state) = first_rays("cornell", gpu)
    out = s.trace_paths(org[:0], d[:0], state[:0], DEPTH)
    assert out["radiance"].shape == (0, 3) and out["rng"].shape == (0,) and out["rays"].shape == (0,)
    s.trace_paths_device(0, 0, 0, 0, 0, DEPTH)  # n == 0: RT_OK whatever the pointers
    whole = s.trace_paths(org, d, state, DEPTH)
    k = 777
    one = s.trace_paths(org[k:k + 1], d[k:k + 1], state[k:k + 1], DEPTH)
    for key in whole:
        np.testing.assert_array_equal(one[key], whole[key][k:k + 1], err_msg=key)


def test_depth_one_is_a_depth_one_frame(gpu):
    sd, s = case_scene("cornell", gpu)
    _, _, w, h = CASES["cornell"]
    cam = Camera.for_scene(sd, (w, h))
    fr = render(MegakernelRenderer, s, cam, w, h, 1, 2)
    assert fr.rays == w * h * 2
    assert_frame(chain(s, cam, w, h, 1, 2, megakernel=True), fr, "depth 1")


def test_empty_scene_returns_the_sky_after_one_ray_and_no_draw(gpu):
    sd = scenes.get_scene("empty")
    s = Scene(sd, device=gpu)
    rng = np.random.default_rng(2)
    n = 300
    org, d = rng.normal(size=(n, 3)).astype(f32), rng.normal(size=(n, 3)).astype(f32)
    state = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    for samples in (1, 2):
        out = s.trace_paths(org, d, state, DEPTH, samples=samples)
        np.testing.assert_array_equal(out["radiance"], np.tile(np.asarray(sd.sky, f32), (n, 1)))  # 1 x (sky + 0), (sky + sky) / 2
        np.testing.assert_array_equal(out["rng"], state)
        assert (out["rays"] == samples).all()
    s.close()


def _device_call(s, org, d, state, depth, samples=1, in_place=False, want_rng=True, want_rays=True, stream=None, rr_start=0):
    """rt_trace_paths_device on torch tensors -> (radiance, rng_out or the rng tensor after the call, rays), numpy; outputs start as 0x55 bytes"""
    import torch
    n = len(org)
    o, di = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    st = torch.from_numpy(state.view(np.int32)).cuda()
    rad = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    st_out = st if in_place else torch.full((n,), 0x55555555, dtype=torch.int32, device="cuda")
    rays = torch.full((n,), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.trace_paths_device(n, o.data_ptr(), di.data_ptr(), st.data_ptr(), rad.data_ptr(), depth, samples=samples, rr_start=rr_start,
                         d_rng_out=st_out.data_ptr() if want_rng else 0, d_rays=rays.data_ptr() if want_rays else 0,
                         stream=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return rad.cpu().numpy(), st_out.cpu().numpy().view(np.uint32), rays.cpu().numpy().view(np.uint32), st.cpu().numpy().view(np.uint32)


def test_the_device_form_marks_rejected_rays_and_traces_the_others(gpu):
    s, (org, d, state) = first_rays("atrium", gpu)
    keep = np.arange(0, 128 * 18, 18)  # 128 rays across the frame
    good = {k: v[keep] for k, v in s.trace_paths(org, d, state, DEPTH, samples=2).items()}
    bad = [5, 77]
    o, di, st = (np.insert(a[keep], bad, a[keep][:2], axis=0) for a in (org, d, state))
    pos = np.array(bad) + np.arange(2)  # where np.insert put them
    assert len(o) == 130
    o[pos[0]] = [np.nan, 0.0, 0.0]
    o[pos[1]] = [0.0, 1e30, 0.0]  # finite, far outside the contract range
    rad, st_out, rays, st_in = _device_call(s, o, di, st, DEPTH, samples=2)
    assert np.isnan(rad[pos]).all() and (rays[pos] == 0xFFFFFFFF).all()
    np.testing.assert_array_equal(st_out[pos], st[pos])
    rest = np.setdiff1d(np.arange(130), pos)
    np.testing.assert_array_equal(rad[rest], good["radiance"])
    np.testing.assert_array_equal(st_out[rest], good["rng"])
    np.testing.assert_array_equal(rays[rest], good["rays"])
    np.testing.assert_array_equal(st_in, st)  # rng_out elsewhere: the input states are read only
    with pytest.raises(abi.RtError) as e:  # the host form refuses the call and names the first rejected ray
        s.trace_paths(o, di, st, DEPTH)
    assert e.value.status == abi.RT_ERR_INVALID and f"ray {pos[0]}:" in str(e.value)


def test_states_in_place_and_outputs_left_out(gpu):
    s, (org, d, state) = first_rays("cornell", gpu)
    org, d, state = org[:700], d[:700], state[:700]
    want = s.trace_paths(org, d, state, DEPTH)
    rad, st_out, rays, _ = _device_call(s, org, d, state, DEPTH, in_place=True)  # rng_out == rng
    np.testing.assert_array_equal(rad, want["radiance"])
    np.testing.assert_array_equal(st_out, want["rng"])
    np.testing.assert_array_equal(rays, want["rays"])
    rad, st_out, rays, st_in = _device_call(s, org, d, state, DEPTH, want_rng=False, want_rays=False)  # both NULL
    np.testing.assert_array_equal(rad, want["radiance"])
    assert (st_out == 0x55555555).all() and (rays == 0x55555555).all()
    np.testing.assert_array_equal(st_in, state)


# ---- 6. streams and updates ---------------------------------------------------------------------------------------------------------------------
def test_update_waits_for_a_pending_path_query(gpu):
    """A device-form query on a non-null stream behind a long kernel, then rt_scene_update: the query returns what the scene held before."""
    import torch
    from test_scene_update import spin_about_centre
    sd, _ = case_scene("atrium", gpu)
    _, _, w, h = CASES["atrium"]
    s = Scene(sd, device=gpu, updatable=True)
    _, (org, d, state) = first_rays("atrium", gpu)
    before = s.trace_paths(org, d, state, DEPTH)
    n = len(org)
    st = torch.cuda.Stream(device=0)
    o, di = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    a = torch.from_numpy(state.view(np.int32)).cuda()
    rad = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    rays = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)  # ~0.1 s of spinning in front of the query
    s.trace_paths_device(n, o.data_ptr(), di.data_ptr(), a.data_ptr(), rad.data_ptr(), DEPTH, d_rng_out=a.data_ptr(), d_rays=rays.data_ptr(),
                         stream=st.cuda_stream)
    s.update(instances=spin_about_centre(sd, 25.0))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rad.cpu().numpy(), before["radiance"])
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), before["rng"])
    np.testing.assert_array_equal(rays.cpu().numpy().view(np.uint32), before["rays"])
    fresh = Scene(s.desc, device=gpu)
    after = s.trace_paths(org, d, state, DEPTH)
    moved = fresh.trace_paths(org, d, state, DEPTH)
    assert not np.array_equal(moved["radiance"], before["radiance"])  # the update did move the scene
    for k in moved:
        np.testing.assert_array_equal(after[k], moved[k], err_msg=k)
    fresh.close(), s.close()


def test_a_ray_query_and_a_path_query_back_to_back_on_two_streams(gpu):
    """They share the scene's ray cursors: the later launch waits for the earlier one on the device, and each returns what it returns alone."""
    import torch
    s, (org, d, state) = first_rays("atrium", gpu)
    n = len(org)
    alone_t = s.trace(org, d)
    alone_p = s.trace_paths(org, d, state, DEPTH)
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    o, di = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    a = torch.from_numpy(state.view(np.int32)).cuda()
    for path_first in (False, True):
        t = torch.zeros(n, dtype=torch.float32, device="cuda")
        tri = torch.zeros(n, dtype=torch.int32, device="cuda")
        rad = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        a_out = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(50_000_000)
        calls = [lambda st: s.trace_device(n, o.data_ptr(), di.data_ptr(), d_t=t.data_ptr(), d_tri=tri.data_ptr(), stream=st.cuda_stream),
                 lambda st: s.trace_paths_device(n, o.data_ptr(), di.data_ptr(), a.data_ptr(), rad.data_ptr(), DEPTH, d_rng_out=a_out.data_ptr(),
                                                 stream=st.cuda_stream)]
        if path_first:
            calls.reverse()
        calls[0](sa), calls[1](sb)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(t.cpu().numpy(), alone_t[0])
        np.testing.assert_array_equal(tri.cpu().numpy().view(np.uint32), alone_t[3])
        np.testing.assert_array_equal(rad.cpu().numpy(), alone_p["radiance"])
        np.testing.assert_array_equal(a_out.cpu().numpy().view(np.uint32), alone_p["rng"])


# ---- 7. rays no camera produces, against the oracle's path query -----------------------------------------------------------------------------
def assert_result(got, want, what):
    for k in ("radiance", "rng", "rays"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("rr_start", [0, 2])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_the_probe_mix_equals_the_oracle(gpu, name, samples, rr_start):
    _, s = case_scene(name, gpu)
    org, d, state = probe_case(name)[2]
    assert_result(s.trace_paths(org, d, state, DEPTH, samples=samples, rr_start=rr_start), probe_expected(name, DEPTH, samples, rr_start),
                  f"{name}, samples {samples}, rr_start {rr_start}")


def test_the_probe_mix_equals_the_oracle_in_the_device_form(gpu):
    _, s = case_scene("atrium", gpu)
    org, d, state = probe_case("atrium")[2]
    rad, st_out, rays, st_in = _device_call(s, org, d, state, DEPTH, samples=3, rr_start=2)
    assert_result({"radiance": rad, "rng": st_out, "rays": rays}, probe_expected("atrium", DEPTH, 3, 2), "device form")
    np.testing.assert_array_equal(st_in, state)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 2047, 2049])
def test_prefixes_of_the_mix_around_the_shard_and_chunk_sizes(gpu, n):
    """The first n entries: shard k of the 32 holds entries [n k / 32, n (k + 1) / 32). Below 32 most shards are empty, at 32 each holds one
    ray, at 33 one holds two; 63, 64 and 65 lie around a wave and a chunk; 2047 and 2049 around 64 rays per shard (shards of 63 and 64, of
    64 and 65: a chunk that fills a shard exactly, and one ray behind it). An entry's result depends on its own three inputs alone."""
    _, s = case_scene("atrium", gpu)
    org, d, state = probe_case("atrium")[2]
    want = {k: v[:n] for k, v in probe_expected("atrium", DEPTH, 3, 2).items()}
    assert_result(s.trace_paths(org[:n], d[:n], state[:n], DEPTH, samples=3, rr_start=2), want, f"n = {n}")


@pytest.mark.parametrize("name", ["cornell", "tables"])
def test_directions_that_round_to_zero_or_overflow_half_return_the_sky(gpu, name):
    """All three components below half's smallest subnormal (the stored direction is zero), and a component past half's largest value (it
    is stored as infinity), among ordinary entries and from inside the Cornell box: the triangle test rejects every triangle for both
    (det == 0; t = 0 or NaN), so each path is the sky after one ray and no draw (tests/test_path_oracle.py checks that of the oracle). The
    Cornell box's sky is black; the table scene's is not."""
    sd, s = case_scene(name, gpu)
    osc = probe_case(name)[1]
    org, d, state = (a[:200].copy() for a in probe_case(name)[2])
    zero, over = [7, 64, 131], [0, 63, 199]
    d[zero] = np.array([[1e-9, -1e-9, 1e-9], [0.0, -0.0, 2e-8], [-1e-9, 1e-30, 0.0]], f32)
    d[over] = np.array([[0.3, 1e5, -0.2], [-7e4, 1.0, 1.0], [65520.0, -65520.0, 1e30]], f32)
    for samples in (1, 2):
        want = osc.trace_paths(org, d, state, DEPTH, samples=samples)
        for k in zero + over:
            np.testing.assert_array_equal(want["radiance"][k], np.asarray(sd.sky, f32))
            assert want["rays"][k] == samples and want["rng"][k] == state[k]
        assert_result(s.trace_paths(org, d, state, DEPTH, samples=samples), want, f"samples {samples}")


# ---- 8. a grid far smaller than the ray list: every wave refills mid-flight -------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3])
def test_a_grid_of_one_and_of_three_workgroups_traces_the_whole_mix(gpu, devlib, monkeypatch, grid):
    """RT_PATH_GRID (developer library only) caps the persistent grid. With one workgroup eight waves share the mix's 65 chunks: every
    wave takes new rays beside live ones many times, hands a claimed chunk out in parts over several rounds, reuses its lanes for entry
    after entry and walks all 32 shards. 3 does not divide 32: the workgroups start on shards 0, 1 and 2."""
    monkeypatch.setenv("RT_PATH_GRID", str(grid))
    sd, product = case_scene("atrium", gpu)
    small = Scene(sd, device=gpu, lib=devlib)  # the knob is read at this scene's first path query
    org, d, state = probe_case("atrium")[2]
    assert len(org) == PROBE_N > 8 * grid * 64 * 2
    for rr_start in (0, 2):
        got = small.trace_paths(org, d, state, DEPTH, samples=2, rr_start=rr_start)
        assert_result(got, probe_expected("atrium", DEPTH, 2, rr_start), f"grid {grid}, rr_start {rr_start}: oracle")
        assert_result(got, product.trace_paths(org, d, state, DEPTH, samples=2, rr_start=rr_start), f"grid {grid}, rr_start {rr_start}: product")
    small.close()


# ---- 9. the size at which the product's own grid is the smaller ----------------------------------------------------------------------------------
FULL_N = (1 << 20) + 17


def test_a_ray_list_larger_than_the_persistent_grid(gpu):
    """2^20 + 17 entries: the mix's entries tiled in a shuffled order, so the expected value is the oracle's result of the mix, indexed.
    The grid is the resident workgroups, 3 per CU (the LDS figure tests/test_path_query.py checks), of 512 lanes each: above that many
    rays the launch stops growing and the waves live on refills. Once through the host form, once through the device form with rejected
    origins spread over the list: a rejected ray leaves its lane idle inside the refill loop."""
    import torch
    _, s = case_scene("atrium", gpu)
    assert FULL_N > torch.cuda.get_device_properties(gpu).multi_processor_count * 3 * 512
    org, d, state = probe_case("atrium")[2]
    want = probe_expected("atrium", DEPTH, 1, 0)
    index = np.arange(FULL_N) % PROBE_N
    np.random.default_rng(23).shuffle(index)
    assert len(np.unique(index[:PROBE_N])) < PROBE_N and len(np.unique(index)) == PROBE_N  # shuffled, and every entry of the mix is there
    o, di, st = org[index], d[index], state[index]
    assert_result(s.trace_paths(o, di, st, DEPTH), {k: v[index] for k, v in want.items()}, "host form")
    bad = np.array([0, 63, 64, 4097, 393216, 393217, 700001, FULL_N - 65, FULL_N - 1])
    o[bad[0::2]] = [np.nan, 0.0, 0.0]
    o[bad[1::2]] = [0.0, 1e30, 0.0]  # finite, far outside the contract range
    rad, st_out, rays, _ = _device_call(s, o, di, st, DEPTH)
    assert np.isnan(rad[bad]).all() and (rays[bad] == 0xFFFFFFFF).all()
    np.testing.assert_array_equal(st_out[bad], st[bad])
    rest = np.ones(FULL_N, bool)
    rest[bad] = False
    assert_result({"radiance": rad[rest], "rng": st_out[rest], "rays": rays[rest]}, {k: v[index][rest] for k, v in want.items()}, "device form")
