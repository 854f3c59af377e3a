"""Reflection probes on the GPU (include/rt_mi355x.h: rt_reflection_probes_*, the kernels of csrc/rt_reflection.hip), bit for bit against the
numpy model of tests/test_reflection_probe.py: rt_reflection_probes_entries against entries_model, rt_reflection_probes_bake against
bake_model around the CPU oracle's path tracer (OracleScene.trace_paths), rt_reflection_probes_prefilter against prefilter_model on
synthetic captures, rt_reflection_probes_sample against sample_model on baked and on synthetic chains. Every comparison is
assert_array_equal. The shapes are the smallest that reach each branch: size 8 with 2 levels (one level of 96 outputs: a wave and a half)
and size 16 with 3 levels (384 + 96 outputs over 1,536 source texels). k_rf_prefilter as built stages 1,024 source texels at a time, so
the source of size 8 (384) is one piece that is not full and the source of size 16 spans two, the last of them half full."""
import ctypes as C

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import ReflectionProbes, Scene
from test_probe_volume import contract_range_model
from test_reflection_probe import (bake_model, centre_model, chain_texels, entries_model, face_dir_model, level_offset, prefilter_model,
                                   prefilter_outputs_model, sample_model, smooth_level0, zero_state_seed)

pytestmark = pytest.mark.gpu
f32 = np.float32
DEPTH, SEED, MAX_SPT = 5, 11, 3
SHAPES = [(8, 2), (16, 3)]
# two probes per scene: inside the Cornell box, among the tables (fitted to the bounds), anywhere in the empty scene
POSITIONS = {"cornell": np.array([[0.0, 0.1, 0.2], [-0.55, 0.4, -0.3]], f32), "tables": None,
             "empty": np.array([[0.0, 1.0, -2.0], [3.0, 0.25, 0.5]], f32)}


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    yield 0
    for r in _PROBES.values():
        r.close()
    for s in _SCENES.values():
        s.close()
    _PROBES.clear(), _SCENES.clear()


_SCENES, _DESCS, _ORACLES, _PROBES, _BAKED = {}, {}, {}, {}, {}


def desc(name):
    if name not in _DESCS:
        _DESCS[name] = scenes.get_scene(name)
    return _DESCS[name]


def positions_of(name):
    if POSITIONS[name] is not None:
        return POSITIONS[name]
    v = desc(name).world_triangles().reshape(-1, 3).astype(np.float64)
    lo, ext = v.min(0), v.max(0) - v.min(0)
    return np.array([lo + 0.3 * ext, lo + (0.7, 0.8, 0.6) * ext], f32)


def unit_boxes(pos, half=(0.4, 0.5, 0.6)):
    pos = np.asarray(pos, f32)
    return np.ascontiguousarray(np.concatenate([pos - np.asarray(half, f32), pos + np.asarray(half, f32)], 1))


def scene_of(name, gpu):
    if name not in _SCENES:
        _SCENES[name] = Scene(desc(name), device=gpu)
    return _SCENES[name]


def probes_of(name, shape, gpu):
    """one object per scene and shape with room for MAX_SPT samples and with boxes, shared by the tests"""
    if (name, shape) not in _PROBES:
        pos = positions_of(name)
        _PROBES[name, shape] = ReflectionProbes(scene_of(name, gpu), pos, shape[0], shape[1], MAX_SPT, boxes=unit_boxes(pos))
    return _PROBES[name, shape]


def oracle_of(name, oracle):
    if name not in _ORACLES:
        _ORACLES[name] = oracle.OracleScene(desc(name))
    return _ORACLES[name]


def expected_bake(name, shape, oracle, spt, rr_start, clamp):
    """bake_model around the oracle, computed once per case and left unchanged"""
    key = (name, shape, spt, rr_start, clamp)
    if key not in _BAKED:
        chain, stats = bake_model(oracle_of(name, oracle).trace_paths, desc(name), positions_of(name), shape[0], shape[1], spt, DEPTH, rr_start, SEED,
                                  clamp)
        chain.setflags(write=False)
        _BAKED[key] = (chain, stats)
    return _BAKED[key]


def assert_chain_equal(got, want):
    np.testing.assert_array_equal(got.view(np.uint32), np.asarray(want).view(np.uint32))  # bits: a NaN equals itself only so


# ---- 1. entries ------------------------------------------------------------------------------------------------------------------------------
def assert_entries(r, spt, seed):
    want = entries_model(r.positions, r.size, spt, seed)
    got = r.entries(spt, seed)
    for k in ("pos", "dir", "state"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    return want


def test_entries_equal_the_model_and_entry_zero_takes_the_replaced_state(gpu):
    r = ReflectionProbes(scene_of("empty", gpu), np.array([[0.25, -1.0, 3.0], [7.0, 0.5, -2.0]], f32), 8, 2, 3)
    want = assert_entries(r, 3, SEED)  # 2,304 entries: nine workgroups
    assert len(want["state"]) == 2304
    want = assert_entries(r, 3, zero_state_seed())
    assert want["state0"][0] == 0x9E3779B9
    assert_entries(r, 1, 0xFFFFFFFF)  # fewer samples than max_spt
    r.close()


def test_entries_in_the_device_form_with_outputs_left_out(gpu):
    import torch
    r = ReflectionProbes(scene_of("empty", gpu), np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], f32), 8, 2, 3)
    want = entries_model(r.positions, 8, 3, SEED)
    n = 2304
    st = torch.cuda.Stream(device=0)
    for mask in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        pos, d = (torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        state = torch.full((n,), 0x55555555, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.entries_device(3, SEED, pos.data_ptr() * mask[0], d.data_ptr() * mask[1], state.data_ptr() * mask[2], stream=st.cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(pos.cpu().numpy(), want["pos"] if mask[0] else np.full((n, 3), 7.0, f32))
        np.testing.assert_array_equal(d.cpu().numpy(), want["dir"] if mask[1] else np.full((n, 3), 7.0, f32))
        np.testing.assert_array_equal(state.cpu().numpy().view(np.uint32), want["state"] if mask[2] else np.full(n, 0x55555555, np.uint32))
    with pytest.raises(abi.RtError) as e:
        r.entries_device(3, SEED)
    assert e.value.status == abi.RT_ERR_INVALID
    r.close()


# ---- 2. bake against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [0.0, 1.5])
@pytest.mark.parametrize("rr_start", [0, 2])
@pytest.mark.parametrize("spt", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["cornell", "tables", "empty"])
def test_a_bake_is_the_model_around_the_oracles_paths(gpu, oracle, name, shape, spt, rr_start, clamp):
    r = probes_of(name, shape, gpu)
    want, stats = expected_bake(name, shape, oracle, spt, rr_start, clamp)
    chain, got = r.bake(spt, DEPTH, rr_start, SEED, clamp)
    assert_chain_equal(chain, want)
    entries = 2 * 6 * shape[0] ** 2 * spt
    assert got == stats and stats["valid"] == stats["probes"] == 2 and stats["rays"] >= entries
    assert_chain_equal(r.get_chain(), want)  # the chain stays in the object
    assert (chain[..., 3] == 1).all() and (chain[..., :3] > 0).any() and np.isfinite(chain).all()
    if name != "empty":
        assert stats["rays"] > entries
    if clamp:
        assert chain[..., :3].max() <= clamp * (1 + 1e-5)  # (a weighted mean of clamped values, up to its rounding)


def test_three_probes_cover_the_tail_of_the_small_levels(gpu, oracle):
    """One probe's level of faces of 4 gives 96 outputs, a wave and a half; three probes give workgroups with idle waves at both shapes"""
    sd = desc("cornell")
    pos = np.array([[0.0, 0.1, 0.2], [0.5, -0.5, 0.1], [-0.2, 0.6, -0.6]], f32)
    for size, levels in SHAPES:
        r = ReflectionProbes(scene_of("cornell", gpu), pos, size, levels, 1)
        want, stats = bake_model(oracle_of("cornell", oracle).trace_paths, sd, pos, size, levels, 1, DEPTH, 0, SEED)
        chain, got = r.bake(1, DEPTH, 0, SEED)
        assert_chain_equal(chain, want)
        assert got == stats and got["valid"] == 3
        r.close()


def test_a_probe_outside_the_contract_range_is_invalid_and_not_counted(gpu, oracle):
    sd = desc("cornell")
    pos = np.array([[0.0, 0.1, 0.2], [1000.0, 0.0, 0.0], [-0.55, 0.4, -0.3]], f32)
    np.testing.assert_array_equal(contract_range_model(sd)(pos), [True, False, True])
    r = ReflectionProbes(scene_of("cornell", gpu), pos, 8, 2, 3)
    want, stats = bake_model(oracle_of("cornell", oracle).trace_paths, sd, pos, 8, 2, 3, DEPTH, 0, SEED)
    chain, got = r.bake(3, DEPTH, 0, SEED)
    assert_chain_equal(chain, want)
    assert got == stats and got["probes"] == 3 and got["valid"] == 2 and got["rays"] >= 2 * 384 * 3
    assert (chain[1].view(np.uint32) == 0).all() and (chain[[0, 2], :, 3] == 1).all()
    # the other probes are what they are without it
    alone, _ = bake_model(oracle_of("cornell", oracle).trace_paths, sd, pos[:1], 8, 2, 3, DEPTH, 0, SEED)
    assert_chain_equal(chain[0], alone[0])
    d = np.array([[0.3, -1.0, 0.2]] * 2, f32)
    out = r.sample(np.array([1, 0]), d, 0.5)
    assert (out[0] == 0).all() and (out[1] > 0).any()  # an invalid probe samples to zeros
    r.close()


def test_a_probe_inside_a_solid_is_valid_and_equals_the_model(gpu, oracle):
    sd = desc("cornell")
    pos = np.array([[-0.35, -0.4, -0.3]], f32)  # the centre of the metal box
    r = ReflectionProbes(scene_of("cornell", gpu), pos, 8, 2, 3)
    want, stats = bake_model(oracle_of("cornell", oracle).trace_paths, sd, pos, 8, 2, 3, DEPTH, 0, SEED)
    chain, got = r.bake(3, DEPTH, 0, SEED)
    assert_chain_equal(chain, want)
    assert got == stats and got["valid"] == 1
    r.close()


def test_the_device_form_on_a_stream_with_stats_equals_the_host_form(gpu, oracle):
    import torch
    shape = (16, 3)
    r = probes_of("cornell", shape, gpu)
    want, stats = expected_bake("cornell", shape, oracle, 3, 2, 1.5)
    st = torch.cuda.Stream(device=0)
    for want_chain, want_stats in ((True, True), (False, False)):
        chain = torch.full((2, r.chain_texels, 4), 7.0, dtype=torch.float32, device="cuda")
        words = torch.full((2,), 0x5555555555555555, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        r.bake_device(3, DEPTH, 2, SEED, 1.5, d_chain=chain.data_ptr() if want_chain else 0, d_stats=words.data_ptr() if want_stats else 0,
                      stream=st.cuda_stream)
        torch.cuda.synchronize()
        assert_chain_equal(r.get_chain(), want)
        w = words.cpu().numpy()
        if want_chain:
            assert_chain_equal(chain.cpu().numpy(), want)
            assert {"probes": int(w.view(np.uint32)[0]), "valid": int(w.view(np.uint32)[1]), "rays": int(w.view(np.uint64)[1])} == stats
        else:
            assert (chain.cpu().numpy() == 7.0).all() and (w.view(np.uint32) == 0x55555555).all()
    out = torch.full((2, r.chain_texels, 4), 7.0, dtype=torch.float32, device="cuda")
    r.get_chain_device(out.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert_chain_equal(out.cpu().numpy(), want)


def test_refusals_that_need_an_object(gpu):
    r = ReflectionProbes(scene_of("empty", gpu), np.zeros((2, 3), f32), 8, 2, 2)
    d = np.array([[1.0, 0.0, 0.0]] * 3, f32)
    idx = np.zeros(3, np.uint32)
    for call, what in ((lambda: r.sample(idx, d, 0.0), "sample"), (lambda: r.get_chain(), "get_chain"), (lambda: r.prefilter(), "prefilter"),
                       (lambda: r.prefilter_device(), "prefilter"), (lambda: r.get_chain_device(1 << 20), "get_chain"),
                       (lambda: r.sample_device(3, 1 << 20, 0, 1 << 20, 1 << 20, 1 << 20), "sample")):
        with pytest.raises(abi.RtError) as e:
            call()
        assert e.value.status == abi.RT_ERR_INVALID and "no level 0" in str(e.value) and what in str(e.value)
    for args, word in (((0, 5), "spt"), ((3, 5), "max_spt"), ((2, 0), "max_depth"), ((3, 0), "max_spt"), ((2, 5, 0, 0, -1.0), "clamp"),
                       ((2, 5, 0, 0, float("nan")), "clamp"), ((2, 0, 0, 0, -1.0), "max_depth"), ((0, 0, 0, 0, -1.0), "spt")):
        with pytest.raises(abi.RtError) as e:
            r.bake(*args)
        assert e.value.status == abi.RT_ERR_INVALID and word in str(e.value), (args, str(e.value))
        with pytest.raises(abi.RtError) as e:
            r.bake_device(*args)
        assert e.value.status == abi.RT_ERR_INVALID
    with pytest.raises(abi.RtError):
        r.entries(3, 0)
    p = abi.rt_reflection_bake_params(2, 5, 0, 1, 0.0)
    L = r._lib
    assert L.rt_reflection_probes_entries(r.h, C.byref(p), None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_reflection_probes_set_level0(r.h, None) == abi.RT_ERR_INVALID
    assert L.rt_reflection_probes_get_chain(r.h, None) == abi.RT_ERR_INVALID
    # a level 0 alone: the levels above are stale, sample is refused until a prefilter; get_chain is not
    lv = smooth_level0(2, 8, 1)
    r.set_level0(lv)
    with pytest.raises(abi.RtError) as e:
        r.sample(idx, d, 0.0)
    assert e.value.status == abi.RT_ERR_INVALID and "stale" in str(e.value)
    np.testing.assert_array_equal(r.level(r.get_chain(), 0), lv)
    r.prefilter()
    assert np.isfinite(r.sample(idx, d, 0.0)).all()
    assert L.rt_reflection_probes_sample(r.h, 3, abi.u32ptr(idx), None, None, abi.fptr(d), abi.fptr(d)) == abi.RT_ERR_INVALID
    assert L.rt_reflection_probes_sample(r.h, 0, None, None, None, None, None) == abi.RT_OK  # n == 0: nothing launched
    assert L.rt_reflection_probes_bake(r.h, C.byref(p), None, None) == abi.RT_OK  # both outputs may be left out
    for bad in ((idx, d[:, :2], 0.0), (idx[:2], d, 0.0), (idx.astype(f32), d, 0.0), (idx, d, np.zeros(2, f32)), (idx, d.astype(np.int32), 0.0),
                (idx, d, 0.0, d[:2]), (np.array([0, -1, 0]), d, 0.0)):
        with pytest.raises(ValueError):
            r.sample(*bad)
    for bad in (np.zeros((2, 6, 8, 8, 3), f32), np.zeros((1, 6, 8, 8, 4), f32), np.zeros((2, 6, 8, 8, 4), np.float64)):
        with pytest.raises(ValueError):
            r.set_level0(bad)
    assert r.bake(2, 5)[1]["valid"] == 2  # max_spt itself is allowed
    one = ReflectionProbes(scene_of("empty", gpu), np.zeros((1, 3), f32), 8, 1, 1)  # one level: nothing can be stale
    one.set_level0(smooth_level0(1, 8, 2))
    assert np.isfinite(one.sample(idx[:1], d[:1], 0.0)).all()
    one.close(), r.close()


# ---- 3. prefilter on synthetic captures -----------------------------------------------------------------------------------------------------------
def spiked_level0(count, size, seed, invalid=()):
    """random values plus one texel of 1e30 per probe: a multiplication with zero in place of the skip would show as NaN or inf behind it"""
    lv = smooth_level0(count, size, seed, invalid)
    g = np.random.default_rng(seed + 100)
    for p in range(count):
        if p not in invalid:
            lv[p, g.integers(0, 6), g.integers(0, size), g.integers(0, size), :3] = 1e30
    return lv


@pytest.mark.parametrize("count,invalid", [(3, (1,)), (1, ())], ids=["3-one-invalid", "1"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_set_level0_then_prefilter_equals_the_model(gpu, shape, count, invalid):
    import torch
    size, levels = shape
    r =ReflectionProbes(scene_of("empty", gpu), np.zeros((count, 3), f32), size, levels, 1)
    lv = spiked_level0(count, size, 9, invalid)
    want = prefilter_model(lv, size, levels)
    assert np.isfinite(want).all() and (want[..., :3].max() > 1e20)
    r.set_level0(lv)
    r.prefilter()
    assert_chain_equal(r.get_chain(), want)
    for p in invalid:
        assert (want[p].view(np.uint32) == 0).all()
    # the device forms, on a stream
    st = torch.cuda.Stream(device=0)
    d_lv = torch.from_numpy(lv[::-1].copy()).cuda()  # the probes in the other order: another chain
    out = torch.zeros((count, r.chain_texels, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.set_level0_device(d_lv.data_ptr(), stream=st.cuda_stream)
    r.prefilter_device(stream=st.cuda_stream)
    r.get_chain_device(out.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert_chain_equal(out.cpu().numpy(), want[::-1])
    r.close()


@pytest.mark.parametrize("shape", [(32, 4), (64, 5), (128, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_deeper_lobes_equal_the_model_at_chosen_outputs(gpu, shape):
    """Five, seven and nine squarings exist only in chains of four, five and six levels, whose level 0 is too long for the model's loop:
    64 outputs of every level (the first, the last and 62 between) against the accumulated model, one probe, finite texels"""
    size, levels = shape
    r = ReflectionProbes(scene_of("empty", gpu), np.zeros((1, 3), f32), size, levels, 1)
    lv = spiked_level0(1, size, 13)
    r.set_level0(lv)
    r.prefilter()
    chain = r.get_chain()
    np.testing.assert_array_equal(r.level(chain, 0), lv)
    g = np.random.default_rng(14)
    for l in range(1, levels):
        M = 6 * (size >> l) ** 2
        outs = np.unique(np.concatenate([[0, M - 1], g.integers(0, M, 62)]))
        want = prefilter_outputs_model(lv[0].reshape(-1, 4), size, levels, l, outs)
        np.testing.assert_array_equal(chain[0, level_offset(size, l) + outs].view(np.uint32), want.view(np.uint32), err_msg=f"level {l}")
    assert np.isfinite(chain).all()
    r.close()


# ---- 4. sample ----------------------------------------------------------------------------------------------------------------------------------
def sample_inputs(r, n, seed):
    """n points for r: the six axes, the eight cube corners, the twelve edge midpoints (every tie), face edges (s or t exactly +-1), texel
    centres of level 0, the inputs that give NaNs (a zero direction, non-finite components, an index out of range), then random directions of
    any length; lod at and beyond both ends and fractional; positions inside and outside the boxes -> (idx, pos, dirs, lod)"""
    g = np.random.default_rng(seed)
    S = r.size
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    corners = [[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    mids = [v for a in (-1, 1) for b in (-1, 1) for v in ([a, b, 0], [a, 0, b], [0, a, b])]
    f = g.integers(0, 6, 8)
    edges = face_dir_model(f, np.where(np.arange(8) % 2 == 0, f32(1.0), g.uniform(-1, 1, 8).astype(f32)) * g.choice([-1, 1], 8).astype(f32),
                           np.where(np.arange(8) % 2 == 1, f32(-1.0), g.uniform(-1, 1, 8).astype(f32)))
    fc, xc, yc = g.integers(0, 6, 10), g.integers(0, S, 10), g.integers(0, S, 10)
    centres = face_dir_model(fc, centre_model(xc, S), centre_model(yc, S)) * g.uniform(0.1, 9.0, 10).astype(f32)[:, None]
    fixed = np.concatenate([np.array(axes + corners + mids, f32), edges, centres])
    rest = (g.normal(size=(max(n - len(fixed) - 9, 0), 3)) * g.uniform(1e-3, 1e3)).astype(f32)
    bad = np.array([[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [1, 1, -np.inf], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [0, -0.0, 0]], f32)
    dirs = np.concatenate([bad, fixed, rest])[:n]
    idx = g.integers(0, r.count, n).astype(np.uint32)
    lod = g.uniform(-0.5, r.levels - 0.5, n).astype(f32)
    lod[::7], lod[1::7], lod[2::7], lod[3::7] = 0.0, r.levels - 1, -3.0, r.levels + 2.5
    pos = (r.positions[idx.astype(int) % r.count] + g.uniform(-0.7, 0.7, size=(n, 3))).astype(f32)  # the boxes' half extents are 0.4 .. 0.6
    pos[9:15] = r.positions[idx[9:15].astype(int)]  # on the centre
    idx[4], idx[5], lod[6], lod[7] = r.count, 0xFFFFFFFF, np.nan, np.inf
    pos[8] = pos[9]
    extra = np.array([np.nan, 0, 0], f32)
    if n > 40:
        pos[40] = extra  # a position that is not finite (it counts only where pos is passed)
    return idx, np.ascontiguousarray(pos), np.ascontiguousarray(dirs), lod


def assert_samples(r, chain, n, seed):
    idx, pos, dirs, lod = sample_inputs(r, n, seed)
    seen = []
    for use_pos in (False, True):
        out = r.sample(idx, dirs, lod, pos if use_pos else None)
        want = sample_model(chain, r.size, r.levels, r.positions, r.boxes, idx, pos if use_pos else None, dirs, lod)
        np.testing.assert_array_equal(out, want)
        assert np.isnan(out[:8]).all() and np.isfinite(out[9:40]).all() and (out[9:40] >= 0).all()
        seen.append(out)
    return seen


@pytest.mark.parametrize("n", [1000, 65])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_samples_of_a_baked_chain_equal_the_model(gpu, oracle, shape, n):
    r = probes_of("cornell", shape, gpu)
    want, _ = expected_bake("cornell", shape, oracle, 3, 0, 0.0)
    r.set_level0(np.array(r.level(want, 0)))
    r.prefilter()
    assert_chain_equal(r.get_chain(), want)
    plain, boxed = assert_samples(r, want, n, 3)
    assert not np.array_equal(plain[9:], boxed[9:])  # the boxes move the lookups
    assert (plain[9:40] > 0).any()


@pytest.mark.parametrize("n", [1000, 65])
@pytest.mark.parametrize("levels,boxes,invalid", [(1, True, ()), (2, False, (1,)), (3, True, (0, 2))], ids=["1-level", "2-levels-no-boxes", "3-levels"])
def test_samples_of_synthetic_chains_equal_the_model(gpu, levels, boxes, invalid, n):
    g = np.random.default_rng(4)
    pos = g.uniform(-2, 2, size=(3, 3)).astype(f32)
    r = ReflectionProbes(scene_of("empty", gpu), pos, 16, levels, 1, boxes=unit_boxes(pos) if boxes else None)
    lv = smooth_level0(3, 16, 5, invalid)
    chain = prefilter_model(lv, 16, levels)
    r.set_level0(lv)
    r.prefilter()
    assert_chain_equal(r.get_chain(), chain)
    idx, p, dirs, lod = sample_inputs(r, n, 6)
    plain, boxed = assert_samples(r, chain, n, 6)
    assert boxes or np.array_equal(plain[9:40], boxed[9:40])  # without boxes a position changes nothing (but a NaN one gives NaNs)
    ok = np.isfinite(plain).all(1)
    for q in invalid:
        assert (plain[ok & (idx == q)] == 0).all()
    r.close()


def test_points_outside_their_box_and_boxes_off_their_centre(gpu):
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], f32)
    boxes = np.array([[-1, -1, -1, 2, 0.5, 1], [1.5, 2.5, 3.5, 2, 3, 4]], f32)  # the second does not hold its probe
    r = ReflectionProbes(scene_of("empty", gpu), pos, 8, 2, 1, boxes=boxes)
    lv = smooth_level0(2, 8, 8)
    chain = prefilter_model(lv, 8, 2)
    r.set_level0(lv)
    r.prefilter()
    g = np.random.default_rng(9)
    n = 400
    idx = g.integers(0, 2, n).astype(np.uint32)
    q = g.uniform(-3, 6, size=(n, 3)).astype(f32)
    d = g.normal(size=(n, 3)).astype(f32)
    d[::5] *= np.array([1, 0, 0], f32)  # axis-parallel: two slabs are never left
    q[:3], d[:3], idx[:3] = boxes[0, 3:], np.array([[1, 1, 1], [-1, 0, 0], [-1, -1, -1]], f32), 0  # on a corner: t = 0 keeps r
    lod = g.uniform(0, 1, n).astype(f32)
    out = r.sample(idx, d, lod, q)
    np.testing.assert_array_equal(out, sample_model(chain, 8, 2, pos, boxes, idx, q, d, lod))
    assert np.isfinite(out).all()
    r.close()


def test_the_host_form_stages_more_points_than_one_piece(gpu):
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], f32)
    r = ReflectionProbes(scene_of("empty", gpu), pos, 8, 2, 1, boxes=unit_boxes(pos))
    lv = smooth_level0(2, 8, 10)
    chain = prefilter_model(lv, 8, 2)
    r.set_level0(lv)
    r.prefilter()
    assert_samples(r, chain, 65536 + 65, 11)
    r.close()


# ---- 5. ordering ----------------------------------------------------------------------------------------------------------------------------------
def test_a_sample_on_another_stream_waits_for_the_bake(gpu, oracle):
    import torch
    shape = (16, 3)
    r = probes_of("cornell", shape, gpu)
    want, _ = expected_bake("cornell", shape, oracle, 3, 2, 0.0)
    r.set_level0(smooth_level0(2, 16, 1))  # what a sample that did not wait would read
    r.prefilter()
    idx, pos, dirs, lod = sample_inputs(r, 1000, 5)
    t = [torch.from_numpy(a).cuda() for a in (idx.view(np.int32), pos, dirs, lod)]
    out = torch.full((1000, 3), 7.0, dtype=torch.float32, device="cuda")
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    r.bake_device(3, DEPTH, 2, SEED, stream=sa.cuda_stream)
    r.sample_device(1000, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), out.data_ptr(), stream=sb.cuda_stream)  # no host synchronisation
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), sample_model(want, 16, 3, r.positions, r.boxes, idx, pos, dirs, lod))


def test_a_bake_after_an_update_sees_the_moved_scene(gpu):
    from test_scene_update import spin_about_centre
    sd = desc("cornell")
    s = Scene(sd, device=gpu, updatable=True)
    r = ReflectionProbes(s, POSITIONS["cornell"], 8, 2, 3)
    before, _ = r.bake(3, DEPTH, 0, SEED)
    s.update(instances=spin_about_centre(sd, 25.0))
    after, stats = r.bake(3, DEPTH, 0, SEED)
    fresh = Scene(s.desc, device=gpu)
    r2 = ReflectionProbes(fresh, POSITIONS["cornell"], 8, 2, 3)
    moved, stats2 = r2.bake(3, DEPTH, 0, SEED)
    assert_chain_equal(after, moved)
    assert stats == stats2 and not np.array_equal(after, before)
    r2.close(), r.close(), fresh.close(), s.close()
