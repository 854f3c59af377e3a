"""CPU tests of the pixel slices' logic (csrc/rt_launch.h: SliceCursor; csrc/rt_frame.hip: slice_plan), through the host-only models the
developer library exports: rt_dev_slice_plan (the slice plan both renderers use) and rt_dev_slice_replay (the sliced cursor, claimed by
simulated waves and mapped by the kernels' own SliceCursor). No GPU: a wrong mapping shows here as a slot claimed twice, never or past the
queue — on the GPU it is a lane that waits ~15 s for a state that never comes, or a load and a store out of bounds."""
import ctypes as C

import numpy as np
import pytest

from rtamd import abi

MAX_SLICES = 8


@pytest.fixture(autouse=True)
def _product_plan(monkeypatch):
    # the planner as the product runs it: no developer override of the bounds, no injected loss
    monkeypatch.delenv("RT_MEGA_SLICE_BOUNDS", raising=False)
    monkeypatch.delenv("RT_INJECT_SLICE_LOSS", raising=False)


def plan(lib, spp, want, G):
    n, shift, cuts = C.c_uint32(), C.c_uint32(), C.c_uint64()
    bound = np.zeros(MAX_SLICES, np.uint32)
    abi.check(lib.rt_dev_slice_plan(spp, want, G, C.byref(n), C.byref(shift), C.byref(cuts), abi.u32ptr(bound)), lib)
    return n.value, shift.value, cuts.value, bound


def replay(lib, n, n_slices, bound, n_waves, seed, capped):
    cap = n * n_slices
    slot, first = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
    got = C.c_uint32()
    bound = np.ascontiguousarray(bound, np.uint32)
    abi.check(lib.rt_dev_slice_replay(n, n_slices, abi.u32ptr(bound), n_waves, seed, capped, abi.u32ptr(slot), abi.u32ptr(first), cap,
                                      C.byref(got)), lib)
    assert got.value == cap  # every slot of the cursor is claimed once
    return slot, first


def handed(s, shift, cuts):
    """The kernels' test of whether the sample that ends now (the pixel goes on with sample s) ends a slice: the lane that ENDS a slice."""
    return (s & ((1 << shift) - 1)) == 0 and (cuts >> (s >> shift)) & 1 == 1


def expected_shift(spp):
    shift = 0
    while (spp - 1) >> shift >= 64:
        shift += 1
    return shift


# tiles below, at and above a wave's 64 lanes, the 97 x 61 frame, and an eighth of 1080p
REPLAY_N = list(range(1, 201)) + [255, 256, 257, 4096, 97 * 61, 1920 * 1080 // 8]


@pytest.mark.parametrize("n_slices", range(2, MAX_SLICES + 1))
def test_replayed_cursor_hands_out_every_slice_of_every_pixel_exactly_once(devlib, n_slices):
    for spp in (67, 130):  # shift 1 with a short last unit, shift 2
        n_got, _, _, bound = plan(devlib, spp, n_slices, 2.0)
        assert n_got == n_slices
        firsts = np.concatenate([[0], bound[:n_slices - 1]]).astype(np.uint64)  # b_0 = 0, b_j = bound[j - 1]
        for n in REPLAY_N:
            want = np.sort((np.repeat(np.arange(n, dtype=np.uint64), n_slices) << np.uint64(32)) | np.tile(firsts, n))
            for n_waves in (1, 3, 64):
                for seed in ((1, 2, 3) if n <= 257 else (7,)):
                    slot, first = replay(devlib, n, n_slices, bound, n_waves, seed * 1000003 + n, 1)
                    assert int(slot.max()) < n, (n, n_slices, n_waves, seed)
                    got = np.sort((slot.astype(np.uint64) << np.uint64(32)) | first.astype(np.uint64))
                    assert np.array_equal(got, want), (n, n_slices, n_waves, seed)


def test_uncapped_claims_map_slots_past_a_small_queue(devlib):
    """Without the cap a wave's claim of up to 64 slots crosses two slice boundaries of a 16-pixel tile in 4 slices, and the two-slice
    mapping sends slots past the queue: what k_wf_finish<.., SLICED> then loaded and stored through. The cap is what the test above checks."""
    n_slices, n = 4, 16
    _, _, _, bound = plan(devlib, 67, n_slices, 2.0)
    past = []
    for seed in range(1, 9):
        slot, _ = replay(devlib, n, n_slices, bound, 1, seed, 0)
        past.append(int(slot.max()) >= n)
        slot, _ = replay(devlib, n, n_slices, bound, 1, seed, 1)
        assert int(slot.max()) < n
    # (a draw of claims that never crosses two boundaries maps correctly: seed 2 of these eight)
    assert past[0] and sum(past) >= 6, past


def test_replay_rejects_what_the_kernels_never_see(devlib):
    bound = np.full(MAX_SLICES, 8, np.uint32)
    slot, first, got = np.empty(4, np.uint32), np.empty(4, np.uint32), C.c_uint32()
    for n, n_slices, n_waves in ((0, 2, 1), (4, 0, 1), (4, 9, 1), (4, 2, 0)):
        assert devlib.rt_dev_slice_replay(n, n_slices, abi.u32ptr(bound), n_waves, 1, 1, abi.u32ptr(slot), abi.u32ptr(first), 4,
                                          C.byref(got)) == abi.RT_ERR_INVALID
    # more slots than the output holds: refused, not written past
    assert devlib.rt_dev_slice_replay(4, 2, abi.u32ptr(bound), 1, 1, 1, abi.u32ptr(slot), abi.u32ptr(first), 4, C.byref(got)) == abi.RT_ERR_INVALID


PLAN_SPP = list(range(1, 301)) + [511, 512, 513, 1000, 4096]
PLAN_G = (0.5, 1.25, 1.26, 2.0, 6.0, 50.0)


@pytest.mark.parametrize("want", [-1, 0, 1, *range(2, MAX_SLICES + 1)])
def test_slice_plan_geometry(devlib, want):
    for spp in PLAN_SPP:
        shift = expected_shift(spp)
        unit = 1 << shift
        units = -(-spp // unit)
        for G in PLAN_G:
            n, sh, cuts, bound = plan(devlib, spp, want, G)
            ctx = (spp, want, G, n, sh, cuts, list(bound))
            unsliced = want in (0, 1) or spp < 2 or (want < 0 and G <= 1.25)
            assert (n == 1) == unsliced, ctx
            assert 1 <= n <= MAX_SLICES, ctx
            if want >= 2 and not unsliced:
                assert n == min(want, units), ctx
            if n == 1:
                assert cuts == 0 and sh == 0 and all(int(b) == spp for b in bound), ctx
                continue
            assert sh == shift, ctx
            ends = [int(b) for b in bound[:n - 1]]
            assert all(0 < b < spp and b % unit == 0 for b in ends), ctx
            assert all(a < b for a, b in zip(ends, ends[1:])), ctx
            assert all(int(b) == spp for b in bound[n - 1:]), ctx
            # the lane that ends a slice (cuts, shift) and the lane that takes the next one (bound[]) agree on every sample
            assert [s for s in range(1, spp) if handed(s, sh, cuts)] == ends, ctx


def test_automatic_plan_slices_only_above_one_and_a_quarter_generations(devlib):
    assert plan(devlib, 64, -1, 1.25)[0] == 1
    assert plan(devlib, 64, -1, 1.26)[0] >= 2
    assert plan(devlib, 1, 8, 50.0)[0] == 1  # one sample: nothing to cut
