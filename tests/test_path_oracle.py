"""The oracle's path query (oracle/oracle_rt.cpp: orc_trace_paths, OracleScene.trace_paths) without a GPU. It is the reference
tests/test_gpu_path_query.py holds the device to on rays no camera produces, so it is pinned here to what the renderers are already pinned
to: chained over a frame's pixels it is OracleScene.render bit for bit. The probe mix those GPU tests trace (tests/test_path_query.py:
probe_mix) is checked here for what it has to contain, on the oracle's own results."""
import numpy as np
import pytest

from rtamd import abi, scenes
from test_path_query import PROBE_N, PROBE_SEED, get_ray_model, pixel_seed_model, probe_case, probe_expected, probe_mix, scene_bounds

f32 = np.float32
DEPTH, SPP = 5, 3
FRAMES = {"cornell": ("cornell", {}, 48, 32), "atrium": ("atrium", {"coarse": True}, 64, 36)}


def oracle_chain(osc, cam, w, h, depth, spp, megakernel, rr_start):
    """the frame as a chain of the oracle's path queries: (fp32 frame (h, w, 4), unorm8 image, rays)"""
    ys, xs = np.mgrid[0:h, 0:w]
    x, y = xs.ravel(), ys.ravel()
    state = pixel_seed_model(x, y, w, h, megakernel)
    org = np.tile(np.array(list(cam.center), f32), (w * h, 1))
    total, rays = np.zeros((w * h, 3), f32), 0
    for _ in range(spp):
        d, state = get_ray_model(cam, x, y, state)
        out = osc.trace_paths(org, d, state, depth, samples=1, rr_start=rr_start)
        rad, state = out["radiance"], out["rng"]
        if not megakernel:  # clamp01 on every sample, as the wavefront renderer stores it
            rad = np.fmin(np.fmax(rad, f32(0)), f32(1))
        total = total + rad
        rays += int(out["rays"].astype(np.uint64).sum())
    c = np.sqrt(total / f32(spp))
    frame = np.concatenate([c, np.ones((w * h, 1), f32)], 1).reshape(h, w, 4)
    u8 = np.rint(np.fmin(np.fmax(c, f32(0)), f32(1)) * f32(255)).astype(np.uint8)
    return frame, np.concatenate([u8, np.full((w * h, 1), 255, np.uint8)], 1).reshape(h, w, 4), rays


# ---- 1. the oracle's chain is the oracle's frame ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr_start", [0, 2])
@pytest.mark.parametrize("kind", ["megakernel", "wavefront"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_the_oracles_frame_is_a_chain_of_its_path_queries(oracle, scene_cache, name, kind, rr_start):
    sname, kw, w, h = FRAMES[name]
    sd = scene_cache(sname, **kw)
    osc = probe_case(name)[1]
    cam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    mega = kind == "megakernel"
    f, b, rays = osc.render(cam, abi.RT_RENDERER_MEGAKERNEL if mega else abi.RT_RENDERER_WAVEFRONT, DEPTH, SPP, rr_start=rr_start)
    assert f[..., :3].max() > 0 and rays > w * h * SPP
    frame, image, n_rays = oracle_chain(osc, cam, w, h, DEPTH, SPP, mega, rr_start)
    np.testing.assert_array_equal(frame, f)
    np.testing.assert_array_equal(image, b)
    assert n_rays == rays


# ---- 2. samples, the BVH, the empty scene -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr_start", [0, 2])
def test_samples_is_a_chain_of_single_paths(rr_start):
    _, osc, (org, d, state) = probe_case("cornell")
    one = probe_expected("cornell", DEPTH, 4, rr_start)
    total, rays, st = np.zeros_like(org), np.zeros(len(org), np.uint32), state
    for _ in range(4):
        out = osc.trace_paths(org, d, st, DEPTH, samples=1, rr_start=rr_start)
        total, rays, st = total + out["radiance"], rays + out["rays"], out["rng"]
    np.testing.assert_array_equal(one["radiance"], total / f32(4.0))  # ((r0 + r1) + r2) + r3 over 4.0f
    np.testing.assert_array_equal(one["rng"], st)
    np.testing.assert_array_equal(one["rays"], rays)
    assert rays.max() > 4 and (one["rng"] != state).any()


@pytest.mark.parametrize("name", ["cornell", "atrium", "tables"])
def test_the_bvh_only_culls_on_the_probe_mix(name):
    """R5 on rays that start on surfaces, inside glass and far outside the bounds. The coarse atrium has 235,750 triangles: without the
    BVH the whole mix at depth 5 is some 4e9 triangle tests, over ten seconds on eight threads, so there the first 257 entries of the
    (shuffled) mix stand for it; the two small scenes take all of it."""
    _, osc, (org, d, state) = probe_case(name)
    k = 257 if name == "atrium" else PROBE_N
    want = probe_expected(name, DEPTH, 1, 0)
    brute = osc.trace_paths(org[:k], d[:k], state[:k], DEPTH, use_bvh=False)
    for key in want:
        np.testing.assert_array_equal(brute[key], want[key][:k], err_msg=key)


def test_the_empty_scene_is_the_sky_after_one_ray_and_no_draw(oracle):
    sd = scenes.get_scene("empty")
    osc = oracle.OracleScene(sd)
    g = np.random.default_rng(2)
    n = 300
    org, d = g.normal(size=(n, 3)).astype(f32), g.normal(size=(n, 3)).astype(f32)
    state = g.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    sky = np.asarray(sd.sky, f32)
    for samples in (1, 2, 3):
        want = np.zeros(3, f32)
        for _ in range(samples):
            want = want + sky
        want = want / f32(samples)  # the sky itself for 1 and 2
        for use_bvh in (True, False):
            out = osc.trace_paths(org, d, state, DEPTH, samples=samples, use_bvh=use_bvh)
            np.testing.assert_array_equal(out["radiance"], np.tile(want, (n, 1)))
            np.testing.assert_array_equal(out["rng"], state)
            assert (out["rays"] == samples).all()
    np.testing.assert_array_equal(osc.trace_paths(org, d, state, DEPTH, samples=2)["radiance"], np.tile(sky, (n, 1)))
    out = osc.trace_paths(org[:0], d[:0], state[:0], DEPTH)
    assert out["radiance"].shape == (0, 3) and out["rng"].shape == (0,) and out["rays"].shape == (0,)
    for kw in ({"max_depth": 0}, {"max_depth": 5, "samples": 0}):
        with pytest.raises(ValueError):
            osc.trace_paths(org, d, state, **kw)


@pytest.mark.parametrize("name", ["cornell", "tables"])
def test_degenerate_directions_are_the_sky(name):
    """A direction whose three components round to half zero, and one with a component that overflows half to infinity: mt_hit rejects
    every triangle (det == 0; t = 0 or NaN), so the path is the sky after one ray and no draw, from inside the Cornell box too (whose sky
    is black; the table scene's is not)."""
    sd, osc, (org, d, state) = probe_case(name)
    o, di, st = org[:8].copy(), d[:8].copy(), state[:8].copy()
    di[2] = [1e-9, -1e-9, 1e-9]
    di[5] = [0.3, 1e5, -0.2]
    for use_bvh in (True, False):
        out = osc.trace_paths(o, di, st, DEPTH, samples=2, use_bvh=use_bvh)
        for k in (2, 5):
            np.testing.assert_array_equal(out["radiance"][k], np.asarray(sd.sky, f32))
            assert out["rays"][k] == 2 and out["rng"][k] == st[k]


# ---- 3. the probe mix holds what it is for ---------------------------------------------------------------------------------------------------
def test_probe_mix_is_float32_unrounded_and_reproducible(oracle):
    sd, _, (org, d, state) = probe_case("cornell")
    assert org.shape == d.shape == (PROBE_N, 3) and state.shape == (PROBE_N,)
    assert org.dtype == f32 and d.dtype == f32 and state.dtype == np.uint32
    assert list(state[:4]) == [0, 1, 0x80000000, 0xFFFFFFFF] and (state[4:] != 0).all()
    again = probe_mix(sd, PROBE_N, PROBE_SEED)
    for a, b in zip((org, d, state), again):
        np.testing.assert_array_equal(a, b)
    rounded, _ = oracle.half_roundtrip(d)
    assert (rounded != d).any(1).mean() > 0.9  # the caller's directions are not half values: rounding them is the callee's work
    lo, hi, scale = scene_bounds(sd)
    outside = np.maximum(np.maximum(lo - org, org - hi), 0.0).max(1)
    assert 0.1 < (outside > 0).mean() < 0.15 and outside.max() > 60 * scale and outside.max() <= 90 * scale  # inside the 100 of the contract range
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    assert length.min() < 0.02 and length.max() > 50
    zero = (d == 0).sum(1) == 2  # the axis directions, with both signs of zero beside them
    assert zero.sum() >= 12 and np.signbit(d[zero]).any() and (~np.signbit(d[zero])).any()
    tiny = (np.abs(d) > 0) & (np.abs(d) < 2.0 ** -14)
    assert tiny.any(1).sum() >= 5  # half subnormals
    t1 = f32(1.0 + 2.0 ** -11)
    assert (np.abs(d) == t1).any() and (np.abs(d) == f32(1.0 + 3.0 * 2.0 ** -11)).any()  # ties, both ways to even
    assert float(oracle.half_roundtrip(np.array([t1], f32))[0][0]) == 1.0


@pytest.mark.parametrize("name", ["cornell", "atrium", "tables"])
def test_probe_mix_reaches_what_a_camera_fan_does_not(oracle, name):
    """Conditions on the oracle's results, not measurements: PROBE_N and PROBE_SEED are chosen so that they hold."""
    sd, osc, (org, d, state) = probe_case(name)
    for samples in (1, 3):
        out = probe_expected(name, DEPTH, samples, 0)
        assert np.isfinite(out["radiance"]).all()
        assert (out["rays"] > samples).any()
        assert ((out["rays"] == samples) & (out["rng"] == state)).any()  # the sky at once, every time: no draw
        assert int(probe_expected(name, DEPTH, samples, 2)["rays"].astype(np.uint64).sum()) < int(out["rays"].astype(np.uint64).sum())
    rounded, _ = oracle.half_roundtrip(d)
    _, _, _, tri = osc.intersect(org, rounded, True)
    hit = tri != 0xFFFFFFFF
    assert hit.mean() >= 1.0 / 3.0
    first = np.array([m.type for m in sd.materials])[sd.inst_material[sd.tri_instance[tri[hit]]]]
    assert (first == abi.RT_MAT_DIELECTRIC).sum() >= 10  # paths that start with a refraction or a reflection on glass
    lo, hi, _ = scene_bounds(sd)
    outside = (np.maximum(lo - org, org - hi) > 0).any(1)
    assert hit[outside].any() and (~hit[outside]).any()  # far origins aimed at the scene and away from it
