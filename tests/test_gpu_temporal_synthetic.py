"""GPU tests of rt_temporal_accumulate[_device] on generated inputs at the edges of its contract (include/rt_mi355x.h, steps 1-6): the exact
plane steps, the analytic room, its camera path and the injection table of tests/test_temporal.py, whose CPU tests hold the generators and the
model to account. Every comparison here is bit for bit, at every call, of all three outputs, against temporal_model carrying its own history;
the plane steps are compared with the hand-derived answers as well."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from rtamd import abi
from rtamd.renderer import TemporalAccumulator, temporal_params
from test_gpu_temporal import same_bits
from test_temporal import (PLANE_SIZES, PLANE_STEPS, ROOM_PARAMS, _edge, frame_of, plane_camera, plane_gbuffer, plane_step_by_hand,
                           plane_step_inputs, room_sequence, temporal_model)
from test_svgf import moments_model

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = float("inf")


def cam_of(c):
    """What TemporalAccumulator takes for a camera: an object whose .c is the rt_camera."""
    return SimpleNamespace(c=c)


def first_difference(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.argwhere(a.view(np.uint8).reshape(a.shape[:2] + (-1,)) != b.view(np.uint8).reshape(b.shape[:2] + (-1,)))[:4].tolist()


def step(acc, state, frame, g, cam, params, what):
    """One call on the device and in the model; the three outputs compared; returns (out_f32, out_u8, history_len, the model's state)."""
    o, b, n = acc.accumulate(frame, g, cam_of(cam), **params)
    mo, mb, mn, state = temporal_model(state, frame, g, cam, params["max_history"], params["sigma_position"], params["cos_normal"])
    assert same_bits(n, mn), (what, "history_len", np.argwhere(n != mn)[:4].tolist())
    assert same_bits(o, mo), (what, "out_f32", first_difference(o, mo))
    assert same_bits(b, mb), (what, "out_u8", first_difference(b, mb))
    return o, b, n, state


# ---- 1. the room path --------------------------------------------------------------------------------------------------------------------
ROOM_SIZES = [(97, 43), (64, 4), (65, 5), (3, 1031), (1, 1)]  # around the 64 x 4 tile: a partial tile in x and y, exactly one, one more pixel
PARAM_SETS = [dict(), dict(sigma_position=INF), dict(cos_normal=-1.0), dict(cos_normal=1.0), dict(max_history=1), dict(max_history=2),
              dict(max_history=4096), dict(sigma_position=INF, cos_normal=-1.0)]  # (the last: rows on the principal point are blended)


def _id(p):
    return ",".join(f"{k}={v}" for k, v in p.items()) or "defaults"


def run_room(W, H, params_of_call):
    acc = TemporalAccumulator(0, W, H)
    state, blended, longest = None, 0, 0
    for call, tag, cam, frame, g, _ in room_sequence(W, H):
        p = dict(ROOM_PARAMS, **params_of_call(call))
        _, _, n, state = step(acc, state, frame, g, cam, p, (W, H, call, tag))
        blended, longest = blended + int((n >= 2).sum()), max(longest, int(n.max()))
    acc.close()
    return blended, longest


@pytest.mark.parametrize("params", PARAM_SETS, ids=_id)
@pytest.mark.parametrize("W,H", ROOM_SIZES)
def test_room_path_equals_the_model(rtlib, W, H, params):
    blended, longest = run_room(W, H, lambda call: params)
    cap = dict(ROOM_PARAMS, **params)["max_history"]
    assert longest <= cap and (blended > 0) == (cap > 1)  # (what makes the comparison mean something is asserted on the model:
    #                                                                       tests/test_temporal.py: test_room_path_reaches_every_rule)


def test_room_path_equals_the_model_at_full_hd(rtlib):
    blended, longest = run_room(1920, 1080, lambda call: {})
    assert blended > 1920 * 1080 * 8 and longest > 8


# ---- 2. the exact plane steps: the kernel against the model AND against arithmetic done by hand ---------------------------------------------
@pytest.mark.parametrize("W,H", PLANE_SIZES)
@pytest.mark.parametrize("case", PLANE_STEPS)
def test_plane_steps_equal_the_model_and_the_hand_derived_answer(rtlib, case, W, H):
    (c0, f0, g0), (c1, f1, g1) = plane_step_inputs(case, W, H)
    which, accepted = PLANE_STEPS[case][4:]
    p = dict(max_history=8, sigma_position=0.25, cos_normal=0.9)
    acc = TemporalAccumulator(0, W, H)
    o0, _, n0, st = step(acc, None, f0, g0, c0, p, (case, 0))
    assert same_bits(o0, f0) and (n0 == 1).all()
    o, b, n, _ = step(acc, st, f1, g1, c1, p, (case, 1))
    want_o, want_n = plane_step_by_hand(case, f0, f1)
    edge = _edge(W, H, which)
    assert (n[edge] == (2 if accepted else 1)).all(), n[edge]
    assert same_bits(n, want_n) and same_bits(o, want_o), first_difference(o, want_o)
    if not accepted:
        assert same_bits(o[edge], f1[edge])  # the input's own bits
    acc.close()


# ---- 3. a history followed to the limit ---------------------------------------------------------------------------------------------------
def test_long_history_counts_to_4096_and_obeys_a_changing_cap(rtlib):
    import time
    t0 = time.perf_counter()
    cam = plane_camera(0)
    g = plane_gbuffer(cam)
    acc = TemporalAccumulator(0, cam.width, cam.height)
    p = dict(max_history=4096, sigma_position=0.25, cos_normal=0.9)
    state = None
    for i in range(4100):
        _, _, n, state = step(acc, state, frame_of(i), g, cam, p, i)
        assert (n == min(i + 1, 4096)).all(), (i, n.min(), n.max())
    _, _, n, state = step(acc, state, frame_of(5000), g, cam, dict(p, max_history=4), "cap 4")
    assert (n == 4).all()
    _, _, n, state = step(acc, state, frame_of(5001), g, cam, p, "cap 4096 again")
    assert (n == 5).all()
    acc.reset()
    f = frame_of(5002)
    o, _, n, state = step(acc, None, f, g, cam, p, "after reset")
    assert same_bits(o, f) and (n == 1).all()
    _, _, n, _ = step(acc, state, frame_of(5003), g, cam, p, "after reset + 1")
    assert (n == 2).all()
    acc.close()
    print(f"\nlong history: 4104 calls on the device and in the model in {time.perf_counter() - t0:.1f} s")


# ---- 4. parameters that change from call to call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,seed", [(97, 43, 1), (97, 43, 2), (65, 5, 3)])
def test_room_path_with_parameters_drawn_per_call(rtlib, W, H, seed):
    rng = np.random.default_rng(seed)
    draws = [dict(sigma_position=float(rng.choice([0.25, 0.1, 1.0, INF])), cos_normal=float(rng.choice([0.9, -1.0, 1.0, 0.0])),
                  max_history=int(rng.choice([1, 2, 3, 32, 4096]))) for _ in range(64)]
    assert len({tuple(d.values()) for d in draws[:17]}) > 8
    run_room(W, H, lambda call: draws[call])


# ---- 5. two streams and the host variant on one accumulator -----------------------------------------------------------------------------------
def test_calls_on_two_streams_and_the_host_are_serialised(rtlib):
    """Call i on stream A behind ~0.1 s of spinning, call i + 1 on stream B at once, call i + 2 through the host variant: each has to wait
    for the one before it (an event per call that the next call's stream waits for), so all three equal the model's sequential answers."""
    import torch
    W, H = 97, 43
    p = ROOM_PARAMS
    seq = list(room_sequence(W, H))
    acc = TemporalAccumulator(0, W, H)
    state = None
    for call, tag, cam, frame, g, _ in seq[:2]:
        _, _, _, state = step(acc, state, frame, g, cam, p, call)
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    keys = ("normal", "position", "prev_position")
    held = []  # every tensor lives until the final synchronise
    for i in (2, 5, 8):  # three rounds along the path: a round starts from what the previous round's host call left
        outs = []
        for _, _, cam, frame, g, _ in seq[i:i + 2]:
            t_in = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (frame, *(g[k] for k in keys))]
            t_out = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"), torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0"),
                     torch.zeros((H, W), dtype=torch.float32, device="cuda:0")]
            held.append((t_in, t_out))
            outs.append(t_out)
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(200_000_000)
        for (t_in, t_out), st, (_, _, cam, _, _, _) in zip(held[-2:], (sa, sb), seq[i:i + 2]):
            acc.accumulate_device(cam_of(cam), *(t.data_ptr() for t in t_in), *(t.data_ptr() for t in t_out), stream=st.cuda_stream, **p)
        call, tag, cam, frame, g, _ = seq[i + 2]
        o, b, n = acc.accumulate(frame, g, cam_of(cam), **p)
        torch.cuda.synchronize()
        for k, (_, _, cam_k, frame_k, g_k, _) in enumerate(seq[i:i + 2]):
            mo, mb, mn, state = temporal_model(state, frame_k, g_k, cam_k, **p)
            do, db, dn = (t.cpu().numpy() for t in outs[k])
            assert same_bits(dn, mn) and same_bits(do, mo) and same_bits(db, mb), (i + k, "device call")
        mo, mb, mn, state = temporal_model(state, frame, g, cam, **p)
        assert same_bits(n, mn) and same_bits(o, mo) and same_bits(b, mb), (i + 2, "host call")
        assert (mn >= 2).mean() > 0.5  # (the three calls did depend on each other)
    acc.close()


def test_plain_moments_and_host_calls_on_one_accumulator_share_one_bracket(rtlib):
    """One accumulator with moments, three room frames, no host synchronisation between the calls: rt_temporal_accumulate_device on stream A,
    rt_temporal_accumulate_moments_device on stream B, then the host rt_temporal_accumulate_moments. Each call's stream waits for the event
    behind the call before it, so the three equal the models' sequential answers. 65 x 5: one tile and one pixel more in x and in y."""
    import torch
    W, H = 65, 5
    p = ROOM_PARAMS
    seq = list(room_sequence(W, H))[:3]
    keys = ("normal", "position", "prev_position")
    t_in = [[torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (frame, *(g[k] for k in keys))] for _, _, _, frame, g, _ in seq[:2]]
    t_out = [[torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"), torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0"),
              torch.zeros((H, W), dtype=torch.float32, device="cuda:0")] for _ in range(2)]
    d_mom = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda:0")
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    acc = TemporalAccumulator(0, W, H, moments=True)
    torch.cuda.synchronize()
    acc.accumulate_device(cam_of(seq[0][2]), *(t.data_ptr() for t in t_in[0]), *(t.data_ptr() for t in t_out[0]), stream=sa.cuda_stream, **p)
    acc.accumulate_moments_device(cam_of(seq[1][2]), *(t.data_ptr() for t in t_in[1]), d_mom.data_ptr(), *(t.data_ptr() for t in t_out[1]),
                                  stream=sb.cuda_stream, **p)
    r = acc.accumulate(seq[2][3], seq[2][4], cam_of(seq[2][2]), moments=True, **p)
    torch.cuda.synchronize()
    state = plain = None
    for k, (_, _, cam, frame, g, _) in enumerate(seq):
        mo, mb, mn, mm, state = moments_model(state, frame, g, cam, **p)
        po, pb, pn, plain = temporal_model(plain, frame, g, cam, **p)
        assert same_bits(mo, po) and same_bits(mb, pb) and same_bits(mn, pn), k  # (the moments ride along: the colour is temporal_model's)
        if k < 2:
            do, db, dn = (t.cpu().numpy() for t in t_out[k])
            assert same_bits(dn, mn) and same_bits(do, mo) and same_bits(db, mb), (k, "device call")
        if k == 1:
            assert same_bits(d_mom.cpu().numpy(), mm), "the moments call's moments, blended with those the plain call before it kept"
    assert same_bits(r["history_len"], mn) and same_bits(r["f32"], mo) and same_bits(r["u8"], mb) and same_bits(r["moments"], mm)
    assert mn.max() == 3 and (mn >= 2).mean() > 0.5  # (the three calls did depend on each other)
    acc.close()


# ---- 6. optional outputs and in place, on inputs that hold the edge rows ------------------------------------------------------------------------
def test_null_history_len_u8_only_and_in_place_on_room_calls(rtlib):
    import torch
    W, H = 97, 43
    p = ROOM_PARAMS
    seq = list(room_sequence(W, H))
    acc = TemporalAccumulator(0, W, H)
    state = None
    keys = ("normal", "position", "prev_position")
    for call, tag, cam, frame, g, where in seq[:8]:
        mo, mb, mn, state = temporal_model(state, frame, g, cam, **p)
        t_in = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (frame, *(g[k] for k in keys))]
        d_f = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        d_b = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda:0")
        d_n = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ptr = [t.data_ptr() for t in t_in]
        if call % 4 == 1:    # history_len NULL
            acc.accumulate_device(cam_of(cam), *ptr, d_f.data_ptr(), d_b.data_ptr(), 0, **p)
            torch.cuda.synchronize()
            assert same_bits(d_f.cpu().numpy(), mo) and same_bits(d_b.cpu().numpy(), mb) and (d_n.cpu().numpy() == 7).all(), call
        elif call % 4 == 2:  # out_u8 only
            acc.accumulate_device(cam_of(cam), *ptr, 0, d_b.data_ptr(), d_n.data_ptr(), **p)
            torch.cuda.synchronize()
            assert same_bits(d_b.cpu().numpy(), mb) and same_bits(d_n.cpu().numpy(), mn) and (d_f.cpu().numpy() == 7).all(), call
        elif call % 4 == 3:  # in place on the device
            acc.accumulate_device(cam_of(cam), *ptr, ptr[0], 0, d_n.data_ptr(), **p)
            torch.cuda.synchronize()
            assert same_bits(t_in[0].cpu().numpy(), mo) and same_bits(d_n.cpu().numpy(), mn) and (d_b.cpu().numpy() == 7).all(), call
        else:                # all three, through the host variant with a NULL history_len
            o, b = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), np.uint8)
            pr = temporal_params(**p)
            planes = [np.ascontiguousarray(a, f32) for a in (frame, *(g[k] for k in keys))]
            abi.check(acc._lib.rt_temporal_accumulate(acc.h, C.byref(pr), C.byref(cam), *(abi.fptr(a) for a in planes), abi.fptr(o), abi.u8ptr(b),
                                                      None), acc._lib)
            assert same_bits(o, mo) and same_bits(b, mb), call
        if call >= 1:
            assert where and (mn >= 2).mean() > 0.5, call  # the calls held the injected rows and most pixels a history
    acc.close()
