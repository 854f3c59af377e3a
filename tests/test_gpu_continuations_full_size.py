"""GPU tests of progressive and adaptive continuations at full frame size.

The identity is the one tests/test_gpu_progressive.py and tests/test_gpu_adaptive.py pin on small images: every pixel whose 8x8 block holds n
samples is, bit for bit in the fp32 frame and the unorm8 image, the pixel of a fresh frame of n samples. Small images never leave the paths a
tiny launch takes; here the continuations run where a real frame runs, and every test asserts which path ran:
- the megakernel's dynamic cursor (more listed 8x8 tiles than the device holds waves: > 32 x CUs) and its chain regime (<= 4 x CUs, unsliced),
  with a carried state (CARRY = 2) and with a block list (CARRY = 3);
- automatic pixel slices (Frame.pixel_slices > 1 without a forced count) of shift 0 (<= 64 samples) and shift >= 1 (> 64 samples, the library's
  own slice plan says so);
- the wavefront renderer's one-launch schedule on one stream lane and on more than one (Frame.stream_lanes), and its cost order
  (Frame.cost_ordered);
- the adaptive policy's compaction (k_adapt_compact) over more than 64 and more than 1,024 blocks, exactly, and its error estimate against the
  vectorised float64 model of tests/test_adaptive.py."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer

pytestmark = pytest.mark.gpu
KINDS = [(MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL), (WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT)]
FULL = (1920, 1080)
RAGGED = (1917, 1077)  # still 240 x 135 blocks, the right column 5 pixels wide and the bottom row 5 rows high


def _load(name):
    spec = importlib.util.spec_from_file_location(f"_{name}_helpers", Path(__file__).with_name(f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_model = _load("test_adaptive")
_small = _load("test_gpu_adaptive")
Refs, _check_per_block = _small.Refs, _small._check_per_block
block_errors_vec, block_index_map, block_grid = _model.block_errors_vec, _model.block_index_map, _model.block_grid


@pytest.fixture(scope="module")
def scenes_gpu(rtlib, scene_cache):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = Scene(scene_cache(name, **kw), device=0)
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


@pytest.fixture(scope="module")
def cus():
    torch = pytest.importorskip("torch")
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dynamic(listed, cus):
    """The megakernel hands these tiles out through its frame-wide cursor: more 8x8 tiles than the device holds waves at any occupancy."""
    return listed > 32 * cus


def _chain(listed, cus):
    """... and takes them all at once (the chain regime) when unsliced: no more tiles than 4 waves per CU."""
    return listed <= 4 * cus


def _shift(devlib, spp):
    """The shift of an automatically sliced plan of `spp` samples (rt_frame.hip: slice_plan; it depends on spp alone)."""
    n, shift, cuts = C.c_uint32(), C.c_uint32(), C.c_uint64()
    bound = np.zeros(8, np.uint32)
    abi.check(devlib.rt_dev_slice_plan(spp, -1, 8.0, C.byref(n), C.byref(shift), C.byref(cuts), abi.u32ptr(bound)), devlib)
    assert n.value > 1
    return shift.value


def _assert_schedule(fr, cls, lanes=1):
    if cls is MegakernelRenderer:
        assert fr.kernels["megakernel"] == 1
    else:  # the one-launch schedule
        assert fr.kernels["wf_finish"] >= 1 and fr.kernels["wf_extend"] == 0 and fr.kernels["wf_shoot"] == 0
        if lanes == 1:
            assert fr.stream_lanes == 1
        else:
            assert fr.stream_lanes > 1


def _oracle_strip(oracle, sd, kind, w, h, depth, spp, f32, u8, strip, local_strip=None, what=""):
    """Global 8-row strip `strip` of a frame of `spp` samples, rendered alone by the CPU oracle, against rows local_strip * 8 ... of the
    GPU's images (the strip comparison of tests/test_gpu_parity.py)."""
    osc = oracle.OracleScene(sd)
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    f, b, _ = osc.render(ocam, kind, depth, spp, use_bvh=True, rank=strip, world=(h + 7) // 8, strip_rows=8)
    lk = strip if local_strip is None else local_strip
    gf, gb = f32[lk * 8: lk * 8 + f.shape[0]], u8[lk * 8: lk * 8 + f.shape[0]]
    nbad = int((gf != f).any(-1).sum())
    assert nbad == 0, f"{what}: strip {strip}: {nbad} pixels differ from the oracle"
    np.testing.assert_array_equal(gb, b)


def _ref_frame(cls, gs, size, depth, spp, cam, sched=None, tile=None):
    r = cls(gs, size, depth, spp)
    if sched:
        r.set_schedule(**sched)
    if tile:
        r.set_tile(*tile)
    fr = r.render_frame(cam)
    r.close()
    return fr


# ---- plain continuations: CARRY = 1 (the frame), 2 (each continuation)
PLAIN = [("atrium4_d10", {"detail": 4}, 10, 2, (1, 8, 65), 66),  # the bench workload
         ("atrium1_d10", {"detail": 1}, 10, 1, (129, 2), 100)]


@pytest.mark.parametrize("cls,kind", KINDS)
@pytest.mark.parametrize("label,kw,depth,a,splits,strip", PLAIN, ids=[p[0] for p in PLAIN])
def test_plain_continuations_at_1080p(scenes_gpu, scene_cache, oracle, devlib, cus, cls, kind, label, kw, depth, a, splits, strip):
    """A frame of a samples continued by 1 (unsliced: the megakernel's dynamic cursor), 8 (automatically sliced, shift 0), 65 or 129 (shift
    >= 1) and 2: the final images and the summed rays are those of the fresh frame of the total, and one strip is the CPU oracle's."""
    sd, gs = scene_cache("atrium", **kw), scenes_gpu("atrium", **kw)
    w, h = FULL
    cam = Camera.for_scene(sd, FULL)
    assert _dynamic(block_grid(w, h)[0] * block_grid(w, h)[1], cus)
    r = cls(gs, FULL, depth, a)
    r.set_progressive(True)
    fr = r.render_frame(cam)
    rays, total, seen = fr.rays, a, set()
    for b in splits:
        fr = r.continue_frame(b)
        rays += fr.rays
        total += b
        _assert_schedule(fr, cls)
        if b == 1:
            assert fr.pixel_slices == 1  # unsliced; the megakernel: 32,400 tiles through the cursor
            seen.add("unsliced")
        else:
            assert fr.pixel_slices > 1  # automatic (pixel_slices -1)
            seen.add(f"shift {'0' if _shift(devlib, b) == 0 else '>=1'}")
    assert r.accumulated_samples == total
    r.close()
    assert seen >= ({"unsliced", "shift 0", "shift >=1"} if label == "atrium4_d10" else {"shift >=1"})
    ref = _ref_frame(cls, gs, FULL, depth, total, cam)
    assert rays == ref.rays
    np.testing.assert_array_equal(fr.rgba_f32, ref.rgba_f32)
    np.testing.assert_array_equal(fr.rgba_u8, ref.rgba_u8)
    _oracle_strip(oracle, sd, kind, w, h, depth, total, fr.rgba_f32, fr.rgba_u8, strip, what=f"{label} {cls.__name__} {total} spp")


def test_plain_continuations_in_the_chain_regime(scenes_gpu, cus):
    """The megakernel's chain regime with a carried state: rank 0 of 34 of 1080p in strips of 8 rows (32 rows, 960 tiles), a frame of 2
    continued by 3 and by 1, unsliced, against the fresh frame of 6 of the same tile."""
    gs = scenes_gpu("atrium", detail=1)
    depth, tile = 10, (0, 34, 8)
    cam = Camera.for_scene(gs.desc, FULL)
    r = MegakernelRenderer(gs, FULL, depth, 2)
    r.set_tile(*tile)
    bx, by = r.block_grid()
    assert r.local_rows == 32 and _chain(bx * by, cus)
    r.set_progressive(True)
    rays = r.render_frame(cam).rays
    for b in (3, 1):
        fr = r.continue_frame(b)
        rays += fr.rays
        assert fr.kernels["megakernel"] == 1 and fr.pixel_slices == 1
    r.close()
    ref = _ref_frame(MegakernelRenderer, gs, FULL, depth, 6, cam, tile=tile)
    assert rays == ref.rays
    np.testing.assert_array_equal(fr.rgba_f32, ref.rgba_f32)
    np.testing.assert_array_equal(fr.rgba_u8, ref.rgba_u8)


# ---- block continuations: CARRY = 3, k_blocks_begin / k_blocks_resolve, k_wf_generate_blocks / k_wf_resolve_blocks
def _lists(nb, seed):
    """every block shuffled, a random half shuffled, a contiguous quarter, a random 1/32 outside the half, the last block, nothing."""
    rng = np.random.default_rng(seed)
    half = rng.choice(nb, nb // 2, replace=False)
    rest = np.setdiff1d(np.arange(nb), half)
    return [("every", rng.permutation(nb), 1), ("half", half, 2), ("quarter", np.arange(nb // 3, nb // 3 + nb // 4), 2),
            ("1/32", rng.choice(rest, nb // 32, replace=False), 2), ("last", np.array([nb - 1]), 2), ("empty", np.array([], np.int64), 3)]


BLOCK_CASES = [(MegakernelRenderer, None), (WavefrontRenderer, None), (WavefrontRenderer, dict(stream_lanes=2))]


@pytest.mark.parametrize("size", [FULL, RAGGED], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cls,sched", BLOCK_CASES, ids=["mega", "wf", "wf_lanes2"])
def test_block_continuations_at_full_size(scenes_gpu, cus, cls, sched, size):
    """A frame of 1, then block continuations of every block (shuffled) by 1, a random half by 2, a contiguous quarter by 2, a random 1/32 by 2,
    the last block by 2 and the empty list by 3: every pixel against the fresh frame of its block's total, the host's counts after every call.
    The list of every block reports the rays of a plain continuation and its image."""
    gs = scenes_gpu("atrium", detail=1)
    depth = 3
    cam = Camera.for_scene(gs.desc, size)
    r = cls(gs, size, depth, 1)
    twin = cls(gs, size, depth, 1)
    for x in (r, twin):
        if sched:
            x.set_schedule(**sched)
        x.set_progressive(True)
        x.render_frame(cam)
    bx, by = r.block_grid()
    assert (bx, by) == (240, 135)
    nb = bx * by
    counts = np.full((by, bx), 1, np.uint32)
    lanes = 1 if not sched else 2
    regimes = set()
    for name, lst, b in _lists(nb, seed=size[0]):
        fr = r.continue_blocks(b, lst)
        counts.reshape(-1)[lst] += b
        np.testing.assert_array_equal(r.block_samples(), counts)
        if name == "empty":
            assert fr.rays == 0
            continue
        _assert_schedule(fr, cls, lanes)
        if name == "every":
            plain = twin.continue_frame(b)
            assert fr.rays == plain.rays
            np.testing.assert_array_equal(fr.rgba_f32, plain.rgba_f32)
            np.testing.assert_array_equal(fr.rgba_u8, plain.rgba_u8)
            assert fr.pixel_slices == 1
        if cls is MegakernelRenderer:
            if name in ("every", "half"):
                assert _dynamic(len(lst), cus)
                regimes.add("dynamic, unsliced" if fr.pixel_slices == 1 else "dynamic, sliced")
            if name == "1/32":
                assert _chain(len(lst), cus) and fr.pixel_slices == 1
                regimes.add("chain")
        elif lanes == 1 and name == "half":
            assert fr.pixel_slices > 1
            regimes.add("one lane, sliced")
        elif lanes > 1:
            assert fr.pixel_slices == 1
            regimes.add("lanes")
    twin.close()
    r.close()
    if cls is MegakernelRenderer:
        assert regimes == {"dynamic, unsliced", "dynamic, sliced", "chain"}
    else:
        assert regimes == ({"one lane, sliced"} if lanes == 1 else {"lanes"})
    assert 3 <= len(np.unique(counts)) <= 5
    _check_per_block(fr.rgba_f32, fr.rgba_u8, counts, Refs(cls, gs, size, depth, cam, sched=sched), f"{cls.__name__} {sched} {size}")


@pytest.mark.parametrize("cls,kind", KINDS)
def test_block_continuation_into_device_tensors(scenes_gpu, cls, kind):
    """rt_render_frame_continue_blocks_device on every 7th block and the last (ragged) one, into torch tensors."""
    torch = pytest.importorskip("torch")
    gs = scenes_gpu("atrium", detail=1)
    w, h = RAGGED
    depth = 3
    cam = Camera.for_scene(gs.desc, RAGGED)
    r = cls(gs, RAGGED, depth, 2)
    r.set_progressive(True)
    r.render_frame(cam)
    bx, by = r.block_grid()
    lst = np.random.default_rng(3).permutation(np.r_[np.arange(0, bx * by, 7), bx * by - 1])
    f = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    b = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    fr = r.continue_blocks_device(3, lst, f.data_ptr(), b.data_ptr())
    torch.cuda.synchronize()
    assert fr.rays > 0
    counts = np.full((by, bx), 2, np.uint32)
    counts.reshape(-1)[lst] += 3
    np.testing.assert_array_equal(r.block_samples(), counts)
    _check_per_block(f.cpu().numpy(), b.cpu().numpy(), counts, Refs(cls, gs, RAGGED, depth, cam), f"{cls.__name__} device outputs")
    r.close()


# ---- the policy: k_adapt_errors and k_adapt_compact
def _median_threshold(r):
    """The median of the blocks' current errors (rt_renderer_adapt evaluates without rendering): a threshold that lists about half the blocks."""
    r.adapt(1e30)
    e = r.block_errors()
    return float(np.median(e[np.isfinite(e)]))


def _policy_passes(r, img, passes):
    """continue_adaptive for each (samples, min_samples) of `passes` at the median threshold of the blocks' errors before it (the first pass,
    without snapshots, lists every block); after each, the library's e_B against block_errors_vec within 1e-4 relative, the next evaluation's
    list against the model's active set on every decisive block, strictly ascending and in range, and then continued by the next pass."""
    bx, by = r.block_grid()
    nb = bx * by
    idx = block_index_map(*img.shape[:2])
    before = np.zeros_like(img)
    has_snap = np.zeros((by, bx), bool)
    threshold, expect = 0.0, None
    lengths = []
    for k, (b, ms) in enumerate(passes):
        fr, blocks = r.continue_adaptive(b, threshold, ms)
        if expect is None:
            assert len(blocks) == nb
        else:
            np.testing.assert_array_equal(blocks, expect)  # what the last evaluation listed
        listed = np.zeros(nb, bool)
        listed[blocks] = True
        m = listed[idx]
        before[m] = img[m]
        has_snap.reshape(-1)[blocks] = True
        img = fr.rgba_f32
        counts = r.block_samples()
        if k + 1 == len(passes):
            break
        threshold, ms = _median_threshold(r), passes[k + 1][1]
        expect = r.adapt(threshold, ms)
        got = r.block_errors()
        model = block_errors_vec(img[..., :3].astype(np.float64) ** 2, before, counts, has_snap)
        fin = np.isfinite(model)
        assert (np.isinf(got) == ~fin).all()
        np.testing.assert_allclose(got[fin], model[fin], rtol=1e-4, atol=1e-7)
        act_model = (~fin | (counts < ms) | (model >= threshold)).reshape(-1)
        act = np.zeros(nb, bool)
        act[expect] = True
        decisive = (~fin | (np.abs(model - threshold) > 1e-3)).reshape(-1)
        assert (act[decisive] == act_model[decisive]).all(), f"{int((act != act_model)[decisive].sum())} decisive blocks differ"
        assert (np.diff(expect.astype(np.int64)) > 0).all() and (len(expect) == 0 or expect[-1] < nb)
        lengths.append(len(expect))
    return fr, lengths


@pytest.mark.parametrize("cls,kind", KINDS)
def test_adaptive_policy_at_1080p(scenes_gpu, cls, kind):
    """Four adaptive passes after a frame of 2 on the 1080p atrium: the first lists every block (no snapshots), the others the noisy ones
    (three evaluations checked against the model)."""
    gs = scenes_gpu("atrium", detail=1)
    cam = Camera.for_scene(gs.desc, FULL)
    r = cls(gs, FULL, 6, 2)
    r.set_progressive(True)
    img = r.render_frame(cam).rgba_f32
    nb = np.prod(r.block_grid())
    fr, lengths = _policy_passes(r, img, ((2, 0), (4, 0), (4, 8), (2, 0)))
    assert len(lengths) == 3 and all(1024 < n < nb for n in lengths), lengths  # partial lists: holes in the 32 chunks of 1,024 blocks
    r.close()


def _holes(nb):
    h = {0, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, nb - 1} | set(range(0, nb, 64)) | set(range(0, nb, 1024)) | set(range(63, nb, 1024))
    return np.array(sorted(b for b in h if b < nb))


COMPACT_SIZES = [(FULL, 32400), ((509, 253), 2048), ((325, 197), 1025)]  # 32 chunks of 1,024; exactly two; one and one block


@pytest.mark.parametrize("cls,kind", KINDS)
@pytest.mark.parametrize("size,nb", COMPACT_SIZES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_compaction_lists_exactly_the_blocks_under_min_samples(scenes_gpu, cls, kind, size, nb):
    """rt_renderer_adapt(1e30, min_samples) lists exactly the blocks below min_samples (every block has a snapshot after a plain
    continuation): no float enters the list, so k_adapt_compact is checked exactly — with holes at 0, 63 .. 65, 1023 .. 1025, 2047, 2048, the
    last block, every 64th and every 1024th block, dense and sparse, then a random third."""
    gs = scenes_gpu("atrium", detail=1)
    cam = Camera.for_scene(gs.desc, size)
    r = cls(gs, size, 1, 1)
    r.set_progressive(True)
    r.render_frame(cam)
    bx, by = r.block_grid()
    assert bx * by == nb > 1024
    everything = np.arange(nb)
    np.testing.assert_array_equal(r.adapt(1e30), everything)  # no snapshots yet
    r.continue_frame(1)
    np.testing.assert_array_equal(r.adapt(0.0), everything)
    assert len(r.adapt(1e30)) == 0
    rng = np.random.default_rng(nb)
    holes = _holes(nb)
    counts = np.full(nb, 2, np.uint32)
    third = rng.choice(nb, nb // 3, replace=False)
    for b, lst, dense in ((1, rng.permutation(holes), True), (2, rng.permutation(np.setdiff1d(everything, holes)), False), (1, third, None)):
        r.continue_blocks(b, lst)
        counts[lst] += b
        np.testing.assert_array_equal(r.block_samples().reshape(-1), counts)
        ms = int(counts.max())
        want = np.flatnonzero(counts < ms)
        got = r.adapt(1e30, ms)
        if dense is not False:
            assert len(want) > (1024 if nb >= 2048 else 64)  # (1,025 blocks: the second chunk holds one)
        if dense is True:
            assert np.array_equal(want, np.setdiff1d(everything, holes))
        if dense is False:
            np.testing.assert_array_equal(want, holes)
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(r.adapt(0.0), everything)
    r.close()


# ---- BASELINE.json config 5's own tile
@pytest.mark.parametrize("cls,kind", KINDS)
def test_config5_tile_continued(scenes_gpu, scene_cache, oracle, cls, kind):
    """3840x2160 rank 0 of 8, strips of 8 rows (272 rows, 480 x 34 = 16,320 blocks), depth 16: a frame of 4, a plain continuation of 4, two
    adaptive continuations of 4 — against fresh frames of the same tile, and one strip of the plain continuation against the oracle."""
    sd, gs = scene_cache("atrium", detail=4), scenes_gpu("atrium", detail=4)
    w, h, depth, world = 3840, 2160, 16, 8
    cam = Camera.for_scene(sd, (w, h))
    tile = (0, world, 8)
    r = cls(gs, (w, h), depth, 4)
    r.set_tile(*tile)
    assert r.local_rows == 272 and r.block_grid() == (480, 34)
    r.set_progressive(True)
    fr = r.render_frame(cam)
    rays = fr.rays
    fr = r.continue_frame(4)
    rays += fr.rays
    refs = Refs(cls, gs, (w, h), depth, cam, tile=tile)
    assert rays == refs(8).rays
    np.testing.assert_array_equal(fr.rgba_f32, refs(8).rgba_f32)
    np.testing.assert_array_equal(fr.rgba_u8, refs(8).rgba_u8)
    _oracle_strip(oracle, sd, kind, w, h, depth, 8, fr.rgba_f32, fr.rgba_u8, 64, local_strip=64 // world, what=f"config 5 tile {cls.__name__}")
    listed = []
    for _ in range(2):
        fr, blocks = r.continue_adaptive(4, _median_threshold(r))  # (the plain continuation left a snapshot in every block)
        listed.append(len(blocks))
    assert all(0 < n < 480 * 34 for n in listed), listed
    counts = r.block_samples()
    assert set(np.unique(counts)) == {8, 12, 16}
    _check_per_block(fr.rgba_f32, fr.rgba_u8, counts, refs, f"config 5 tile {cls.__name__}")
    r.close()


# ---- the wavefront renderer's cost order on a continuation
def test_cost_order_on_a_continuation(scenes_gpu):
    """Rank 0 of 2 of 1080p (544 rows of whole blocks, under the cost-order size limit), unsliced: a continuation of 32 samples runs the
    cost-ordered pair of launches and is the fresh frame of 33."""
    gs = scenes_gpu("atrium", detail=1)
    depth, sched, tile = 4, dict(pixel_slices=0), (0, 2, 8)
    cam = Camera.for_scene(gs.desc, FULL)
    r = WavefrontRenderer(gs, FULL, depth, 1)
    r.set_schedule(**sched)
    r.set_tile(*tile)
    assert r.local_rows == 544
    r.set_progressive(True)
    rays = r.render_frame(cam).rays
    fr = r.continue_frame(32)
    rays += fr.rays
    assert fr.cost_ordered and fr.kernels["wf_tile_order"] >= 1 and fr.stream_lanes == 1 and fr.pixel_slices == 1
    r.close()
    ref = _ref_frame(WavefrontRenderer, gs, FULL, depth, 33, cam, sched=sched, tile=tile)
    assert rays == ref.rays
    np.testing.assert_array_equal(fr.rgba_f32, ref.rgba_f32)
    np.testing.assert_array_equal(fr.rgba_u8, ref.rgba_u8)
