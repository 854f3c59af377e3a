"""CPU tests of the temporal stage — the per-frame seed salt (rt_renderer_set_frame_seed), the motion guide (RT_SCENE_KEEP_PREVIOUS,
rt_scene_gbuffer_motion[_device]) and the accumulator (rt_temporal_*) — and the numpy float32 models that tests/test_gpu_temporal.py pins the
device to bit for bit:

    world_vertices_f32  a scene description's world-space vertices with the builder's fp32 expression (SceneDesc.world_triangles() is float64)
    motion_model        prev_position from rt_intersect_batch's hits of the camera's rays and the PREVIOUS description's world vertices
    temporal_model      one call of rt_temporal_accumulate (include/rt_mi355x.h), carrying its own history from call to call

Every numpy operation below is one IEEE binary32 operation on float32 arrays, in the order the contract states (no FMA in numpy)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi
from test_denoise import _listing, coefficient, to_unorm8

REPO = Path(__file__).resolve().parent.parent
EXE = REPO / "sycl-ray-tracer_amd" / "host" / "build" / "raytracer"
f32 = np.float32
INF = float("inf")


# ---- the motion guide --------------------------------------------------------------------------------------------------------------------
def world_vertices_f32(sd) -> np.ndarray:
    """(T, 3, 3) float32: every triangle's world-space vertices as the library computes them (scene_build.cpp: world_vertices, rt_update.hip:
    ((m0*x + m4*y) + m8*z) + m12 with the instance's column-major matrix)."""
    idx = np.asarray(sd.indices, np.int64).reshape(-1, 3)
    m = np.asarray(sd.transforms, f32).reshape(-1, 16)[np.asarray(sd.tri_instance, np.int64)]  # (T, 16)
    p = np.asarray(sd.positions, f32).reshape(-1, 3)[idx]                                        # (T, 3 vertices, 3)
    out = np.zeros(p.shape, f32)
    for a in range(3):
        out[..., a] = ((m[:, None, a] * p[..., 0] + m[:, None, 4 + a] * p[..., 1]) + m[:, None, 8 + a] * p[..., 2]) + m[:, None, 12 + a]
    return out


def motion_model(prev_world, u, v, tri, w, h):
    """prev_position (h, w, 4) of rt_scene_gbuffer_motion, given rt_intersect_batch's (u, v, tri) for the camera's rays (row 0 first) and the
    previous world vertices (T, 3, 3) float32."""
    out = np.zeros((w * h, 4), f32)
    hit = tri != 0xFFFFFFFF
    if hit.any():
        b = np.asarray(prev_world, f32)[tri[hit].astype(np.int64)]
        bu, bv = u[hit].astype(f32), v[hit].astype(f32)
        bw = (f32(1) - bu) - bv
        out[hit, :3] = (b[:, 0] * bw[:, None] + b[:, 1] * bu[:, None]) + b[:, 2] * bv[:, None]
        out[hit, 3] = 1
    return out.reshape(h, w, 4)


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------------
def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def _cam_vectors(cam):
    return tuple(np.array(list(v), f32) for v in (cam.center, cam.pixel00, cam.delta_u, cam.delta_v))


def reproject(prev_cam, Q, W, H):
    """Step 3: (ok, sx, sy) of the points Q (..., >= 3) through the previous call's camera (an rt_camera)."""
    c, p00, du, dv = _cam_vectors(prev_cam)
    with np.errstate(all="ignore"):
        m = _cross(du, dv)
        e = p00 - c
        r = Q[..., :3] - c
        s = _dot3(e, m) / _dot3(r, m)
        ok = np.isfinite(s) & (s > 0)
        h = r * s[..., None] - e
        sx = _dot3(h, du) / _dot3(du, du)
        sy = _dot3(h, dv) / _dot3(dv, dv)
        ok = ok & (sx > f32(-1)) & (sx < f32(W)) & (sy > f32(-1)) & (sy < f32(H))
    return ok, sx, sy


def reproject_s(prev_cam, Q):
    """Step 3's s alone (fp32): dot(e, m) / dot(r, m)."""
    c, p00, du, dv = _cam_vectors(prev_cam)
    with np.errstate(all="ignore"):
        return _dot3(p00 - c, _cross(du, dv)) / _dot3(Q[..., :3] - c, _cross(du, dv))


def temporal_model(state, frame, gbuf, cam, max_history, sigma_position, cos_normal, trace=None):
    """One call of rt_temporal_accumulate. `state`: None (no previous call since create / reset) or what the previous call returned.
    Returns (out_f32 (H, W, 4), out_u8 (H, W, 4), history_len (H, W), new state). `trace`: a dict that receives, where there was a previous
    call, the intermediate values per pixel and per tap (tap order as the contract's)."""
    F = np.asarray(frame, f32)
    H, W = F.shape[:2]
    N, P, Q = (np.asarray(gbuf[k], f32) for k in ("normal", "position", "prev_position"))
    L = F[..., :3] * F[..., :3]
    hit = np.isfinite(P[..., 3])
    Lo = L.copy()
    n_new = np.where(hit, f32(1), f32(0)).astype(f32)
    blended = np.zeros((H, W), bool)
    if state is not None:
        with np.errstate(all="ignore"):
            ok, sx, sy = reproject(state["cam"], Q, W, H)
            ok = ok & hit
            sx, sy = np.where(ok, sx, f32(0)), np.where(ok, sy, f32(0))
            x0f, y0f = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0f, sy - y0f
            gx, gy = f32(1) - fx, f32(1) - fy
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            kx = coefficient(sigma_position)
            wsum = np.zeros((H, W), f32)
            S = np.zeros((H, W, 3), f32)
            n_min = np.full((H, W), np.inf, f32)
            taps = []
            for j in (0, 1):
                for i in (0, 1):
                    tx, ty = x0 + i, y0 + j
                    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                    tx, ty = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    w = (fx if i else gx) * (fy if j else gy)
                    Ct = state["colour"][ty, tx]
                    t_hit = Ct[..., 3] >= 1
                    pos_ok = nrm_ok = np.ones((H, W), bool)
                    if kx != 0:
                        d = state["position"][ty, tx, :3] - Q[..., :3]
                        pos_ok = _dot3(d, d) * kx <= f32(1)
                    if f32(cos_normal) != f32(-1):
                        nrm_ok = _dot3(N, state["normal"][ty, tx]) >= f32(cos_normal)
                    valid = ok & inside & (w > 0) & t_hit & pos_ok & nrm_ok
                    wsum = np.where(valid, wsum + w, wsum)
                    S = np.where(valid[..., None], S + w[..., None] * Ct[..., :3], S)
                    n_min = np.where(valid, np.fmin(n_min, Ct[..., 3]), n_min)
                    taps.append({"inside": inside, "w": w, "hit": t_hit, "pos_ok": pos_ok, "nrm_ok": nrm_ok, "valid": valid, "n": Ct[..., 3]})
            n_next = np.fmin(n_min + f32(1), f32(max_history))
            good = ok & (wsum >= f32(1) / f32(64)) & (n_next != 1)
            Hc = S / wsum[..., None]
            a = f32(1) / n_next
            Lb = Hc + (L - Hc) * a[..., None]
        Lo = np.where(good[..., None], Lb, L).astype(f32)
        n_new = np.where(good, n_next, n_new).astype(f32)
        blended = good
        if trace is not None:  # what the coverage conditions of the synthetic path are stated in (test_room_path_reaches_every_rule)
            trace.update(hit=hit, s=reproject_s(state["cam"], Q), ok=ok, sx=sx, sy=sy, fx=fx, fy=fy, taps=taps, wsum=wsum, n_next=n_next, good=good)
    with np.errstate(all="ignore"):
        rgb = np.where(blended[..., None], np.sqrt(Lo), F[..., :3])
    out = np.concatenate([rgb, np.ones((H, W, 1), f32)], -1).astype(f32)
    u8 = np.concatenate([to_unorm8(out[..., :3]), np.full((H, W, 1), 255, np.uint8)], -1)
    cam_copy = abi.rt_camera()
    C.memmove(C.byref(cam_copy), C.byref(cam), C.sizeof(abi.rt_camera))
    new_state = {"colour": np.concatenate([Lo, n_new[..., None]], -1).astype(f32), "position": P.copy(), "normal": N.copy(), "cam": cam_copy}
    return out, u8, n_new, new_state


# ---- tests -------------------------------------------------------------------------------------------------------------------------------
NEW = ["rt_renderer_set_frame_seed", "rt_scene_gbuffer_motion", "rt_scene_gbuffer_motion_device", "rt_temporal_create", "rt_temporal_destroy",
       "rt_temporal_reset", "rt_temporal_accumulate", "rt_temporal_accumulate_device"]


def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib):
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
        assert name in abi.PROTOTYPES, name
        assert hasattr(rtlib, name) and hasattr(devlib, name), name
    assert "typedef struct rt_temporal_params" in header
    assert re.search(r"#define RT_SCENE_KEEP_PREVIOUS 2u", header) and abi.RT_SCENE_KEEP_PREVIOUS == 2
    assert C.sizeof(abi.rt_temporal_params) == 12
    assert [f[0] for f in abi.rt_temporal_params._fields_] == ["max_history", "sigma_position", "cos_normal"]
    body = re.search(r"typedef struct rt_temporal_params \{(.*?)\} rt_temporal_params;", header, re.S).group(1)
    assert re.findall(r"(?:uint32_t|float) (\w+);", body) == ["max_history", "sigma_position", "cos_normal"]
    assert rtlib.rt_abi_version() == 8 and devlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header


def _err(lib):
    return lib.rt_last_error().decode() if isinstance(lib.rt_last_error(), bytes) else str(lib.rt_last_error())


def test_refusals_come_before_any_device_call(rtlib):
    """Everything the header lists for rt_temporal_* is refused on the arguments alone: no accumulator exists here, the calls carry a null
    handle, and the parameter refusals are told from the handle's by their messages."""
    buf = np.zeros(16, f32)
    ptr = abi.fptr(buf)
    u8 = abi.u8ptr(np.zeros(16, np.uint8))
    out = C.c_void_p()
    inv = abi.RT_ERR_INVALID
    assert rtlib.rt_temporal_create(-1, 4, 4, C.byref(out)) == inv and not out.value
    assert rtlib.rt_temporal_create(0, 0, 4, C.byref(out)) == inv
    assert rtlib.rt_temporal_create(0, 4, -1, C.byref(out)) == inv
    assert rtlib.rt_temporal_create(0, 4, 4, None) == inv
    assert rtlib.rt_temporal_create(0, 65536, 32768, C.byref(out)) == inv  # W * H = 2^31
    assert rtlib.rt_temporal_create(0, 1, 2**31 - 1, C.byref(out)) == inv  # the 1-D grid of 64 x 4 tiles would pass 2^32 threads
    assert rtlib.rt_temporal_reset(None) == inv
    rtlib.rt_temporal_destroy(None)
    cam = abi.rt_camera()
    cam.width, cam.height = 2, 2
    good = abi.rt_temporal_params(8, 1.0, 0.5)
    for host in (True, False):
        def call(p, f=ptr, o=ptr, b=u8):
            if host:
                return rtlib.rt_temporal_accumulate(None, p, C.byref(cam), f, ptr, ptr, ptr, o, b, None)
            return rtlib.rt_temporal_accumulate_device(None, p, C.byref(cam), 1 if f else None, 1, 1, 1, 1 if o else None, 1 if b else None, None, None)
        assert call(C.byref(good)) == inv and "null argument" in _err(rtlib)
        assert call(None) == inv and "parameters" in _err(rtlib)
        for mh in (0, 4097, 2**32 - 1):
            assert call(C.byref(abi.rt_temporal_params(mh, 1.0, 0.5))) == inv and "max_history" in _err(rtlib), mh
        for s in (0.0, 1e-7, -1.0, float("nan"), -INF):
            assert call(C.byref(abi.rt_temporal_params(8, s, 0.5))) == inv and "sigma_position" in _err(rtlib), s
        for c in (float("nan"), -1.0001, 1.0001, INF):
            assert call(C.byref(abi.rt_temporal_params(8, 1.0, c))) == inv and "cos_normal" in _err(rtlib), c
        assert call(C.byref(good), o=None, b=None) == inv and "both null" in _err(rtlib)
        for ok in (abi.rt_temporal_params(1, INF, -1.0), abi.rt_temporal_params(4096, 1e-6, 1.0)):  # the limits themselves pass the parameter test
            assert call(C.byref(ok)) == inv and "null argument" in _err(rtlib)
    assert rtlib.rt_renderer_set_frame_seed(None, 3) == inv
    assert rtlib.rt_scene_gbuffer_motion(None, C.byref(cam), ptr, ptr, ptr, ptr) == inv
    assert rtlib.rt_scene_gbuffer_motion_device(None, C.byref(cam), 1, 1, 1, 1, None) == inv


def test_keep_previous_needs_updatable_and_a_device(rtlib, scene_cache):
    from rtamd.renderer import Camera, Scene
    sd = scene_cache("cube")
    c = sd.to_c()
    out = C.c_void_p()
    assert rtlib.rt_scene_create_ex(C.byref(c), -1, abi.RT_BVH_DEFAULT, abi.RT_SCENE_KEEP_PREVIOUS, C.byref(out)) == abi.RT_ERR_INVALID and not out.value
    assert rtlib.rt_scene_create_ex(C.byref(c), -1, abi.RT_BVH_DEFAULT, 4, C.byref(out)) == abi.RT_ERR_INVALID
    with pytest.raises(abi.RtError) as e:
        Scene(sd, device=-1, keep_previous=True)
    assert e.value.status == abi.RT_ERR_INVALID
    cam = Camera.for_scene(sd, (4, 3))
    for kw in (dict(updatable=True, keep_previous=True), dict(updatable=True), {}):
        s = Scene(sd, device=-1, **kw)  # a host-only scene: the device is asked for before the flag
        with pytest.raises(abi.RtError) as e:
            s.gbuffer_motion(cam)
        assert e.value.status == abi.RT_ERR_NO_DEVICE, kw
        s.close()
    s = Scene(sd, device=-1, updatable=True, keep_previous=True)  # ... and is still updated on the host
    from test_scene_update import spin_about_centre
    s.update(instances=spin_about_centre(sd, 10.0))
    s.check_bvh()
    s.close()


def test_world_vertices_and_motion_model(scene_cache):
    sd = scene_cache("cornell")
    wv = world_vertices_f32(sd)
    assert wv.dtype == f32 and wv.shape == (sd.n_triangles, 3, 3)
    assert np.allclose(wv, sd.world_triangles(), rtol=1e-5, atol=1e-5)
    tri = np.array([0, 0xFFFFFFFF, 2, 1], np.uint32)
    u = np.array([0, 0, 1, 0], f32)
    v = np.array([0, 0, 0, 1], f32)
    m = motion_model(wv, u, v, tri, 2, 2).reshape(4, 4)
    assert np.array_equal(m[0], [*wv[0, 0], 1]) and np.array_equal(m[1], [0, 0, 0, 0])  # the corners of the barycentric triangle, a miss
    assert np.array_equal(m[2], [*wv[2, 1], 1]) and np.array_equal(m[3], [*wv[1, 2], 1])


# ---- the model on a fronto-parallel plane: exact arithmetic -------------------------------------------------------------------------------
W_, H_ = 24, 10
DU, DV = f32(2.0 ** -4), f32(2.0 ** -4)


def plane_camera(shift_px, W=W_, H=H_, shift_py=0.0):
    """A camera looking down -z at the plane z = -1 (its own image plane, so P = the pixel centre and t = 1), moved sideways by `shift_px`
    pixel steps (and by `shift_py` pixel steps towards later rows). du, dv are powers of two and every coordinate a small multiple of them:
    the model's arithmetic is exact."""
    cam = abi.rt_camera()
    cx, cy = float(shift_px) * float(DU), 0.0 - float(shift_py) * float(DV)
    cam.center[:] = [cx, cy, 0.0]
    cam.pixel00[:] = [cx - (W / 2) * float(DU), cy + (H / 2) * float(DV), -1.0]
    cam.delta_u[:] = [float(DU), 0.0, 0.0]
    cam.delta_v[:] = [0.0, -float(DV), 0.0]
    cam.width, cam.height = W, H
    return cam


def plane_gbuffer(cam, miss=None, n_flip=None):
    W, H = int(cam.width), int(cam.height)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    P = np.zeros((H, W, 4), f32)
    P[..., 0] = f32(cam.pixel00[0]) + xs.astype(f32) * DU
    P[..., 1] = f32(cam.pixel00[1]) - ys.astype(f32) * DV
    P[..., 2] = -1
    P[..., 3] = 1
    N = np.zeros((H, W, 4), f32)
    N[..., 2] = 1
    Q = P.copy()
    if n_flip is not None:
        N[:, n_flip, :3] = (1, 0, 0)
    if miss is not None:
        P[miss] = (0, 0, 0, np.inf)
        N[miss] = 0
        Q[miss] = 0
    return {"normal": N, "position": P, "prev_position": Q}


def frame_of(seed, W=W_, H=H_):
    rng = np.random.default_rng(seed)
    f = np.ones((H, W, 4), f32)
    f[..., :3] = rng.integers(0, 64, (H, W, 3)).astype(f32) / f32(32)  # multiples of 1/32 in [0, 2): squares are exact
    return f


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_model_reprojects_a_sideways_step_onto_single_taps():
    k = 3
    prev, cur = plane_camera(0), plane_camera(k)
    g = plane_gbuffer(cur)
    ok, sx, sy = reproject(prev, g["prev_position"], W_, H_)
    ys, xs = np.meshgrid(np.arange(H_), np.arange(W_), indexing="ij")
    assert np.array_equal(sx, (xs + k).astype(f32)) and np.array_equal(sy, ys.astype(f32))  # exact, as promised
    assert np.array_equal(ok, xs + k < W_)
    f0, f1 = frame_of(1), frame_of(2)
    _, _, n0, st = temporal_model(None, f0, plane_gbuffer(prev), prev, 8, 0.25, 0.9)
    assert (n0 == 1).all()
    o1, u1, n1, st1 = temporal_model(st, f1, g, cur, 8, 0.25, 0.9)
    seen = xs + k < W_
    assert (n1[seen] == 2).all() and (n1[~seen] == 1).all()
    # a single tap of weight 1: the history is exactly the previous frame's pixel k columns to the right, the blend exactly the mean
    L0, L1 = f0[..., :3] * f0[..., :3], f1[..., :3] * f1[..., :3]
    want = np.roll(L0, -k, axis=1) + (L1 - np.roll(L0, -k, axis=1)) * f32(0.5)
    assert np.array_equal(st1["colour"][..., :3][seen], want[seen])
    # the columns that entered the image: output == input bit for bit, history restarted
    assert np.array_equal(bits(o1)[~seen], bits(f1)[~seen])
    assert np.array_equal(bits(st1["colour"][..., :3])[~seen], bits(L1)[~seen])
    assert np.array_equal(u1[..., :3][~seen], to_unorm8(f1[..., :3])[~seen]) and (u1[..., 3] == 255).all()


def test_model_history_length_counts_up_to_the_cap_and_stays():
    cam = plane_camera(0)
    g = plane_gbuffer(cam)
    st, lens = None, []
    for i in range(9):
        _, _, n, st = temporal_model(st, frame_of(i), g, cam, 5, 0.25, 0.9)
        assert (n == n[0, 0]).all()
        lens.append(int(n[0, 0]))
    assert lens == [1, 2, 3, 4, 5, 5, 5, 5, 5]
    # the running mean of a constant sequence is the constant
    st = None
    for i in range(6):
        o, _, _, st = temporal_model(st, frame_of(42), g, cam, 32, 0.25, 0.9)
    assert np.array_equal(o, frame_of(42))


def test_model_thresholds_reset_and_switch_off():
    cam = plane_camera(0)
    cols = slice(5, 9)
    base = plane_gbuffer(cam)
    _, _, _, st = temporal_model(None, frame_of(1), base, cam, 8, 0.25, 0.9)
    f = frame_of(2)
    # a position step beyond sigma resets those columns; with the test off (+inf) it is accepted. (The point moves along its own ray, half
    # as far again: it projects onto its own pixel, at least 0.5 away in space from what the history holds there; sigma is 0.25.)
    g = plane_gbuffer(cam)
    g["prev_position"][:, cols, :3] *= f32(1.5)
    o, _, n, _ = temporal_model(st, f, g, cam, 8, 0.25, 0.9)
    assert (n[:, cols] == 1).all() and (np.delete(n, np.r_[cols], axis=1) == 2).all()
    assert np.array_equal(bits(o[:, cols]), bits(f[:, cols]))
    _, _, n, _ = temporal_model(st, f, g, cam, 8, INF, 0.9)
    assert (n == 2).all()
    # a normal step beyond the threshold resets; cos_normal = -1 accepts (even an opposite normal, whose dot rounds to -1 or below)
    g = plane_gbuffer(cam, n_flip=cols)
    _, _, n, _ = temporal_model(st, f, g, cam, 8, 0.25, 0.9)
    assert (n[:, cols] == 1).all() and (np.delete(n, np.r_[cols], axis=1) == 2).all()
    g["normal"][:, cols, :3] = (0, 0, -1)
    _, _, n, _ = temporal_model(st, f, g, cam, 8, 0.25, -1.0)
    assert (n == 2).all()
    _, _, n, _ = temporal_model(st, f, g, cam, 8, 0.25, -0.999)
    assert (n[:, cols] == 1).all()


def test_model_max_history_one_is_the_identity():
    cam = plane_camera(0)
    g = plane_gbuffer(cam)
    st = None
    for i in range(3):
        f = frame_of(i)
        o, u, n, st = temporal_model(st, f, g, cam, 1, 0.25, 0.9)
        assert np.array_equal(bits(o), bits(f)) and (n == 1).all()
        assert np.array_equal(u[..., :3], to_unorm8(f[..., :3]))


def test_model_a_miss_has_no_length_and_never_serves_as_a_tap():
    prev, cur = plane_camera(0), plane_camera(1)
    miss = np.zeros((H_, W_), bool)
    miss[:, 10] = True
    f0, f1 = frame_of(3), frame_of(4)
    o0, _, n0, st = temporal_model(None, f0, plane_gbuffer(prev, miss=miss), prev, 8, 0.25, 0.9)
    assert (n0[miss] == 0).all() and (n0[~miss] == 1).all() and np.array_equal(bits(o0), bits(f0))
    # one step to the side: column 9 of the new frame looks at what was column 10, the miss: no history there
    o1, _, n1, _ = temporal_model(st, f1, plane_gbuffer(cur), cur, 8, 0.25, 0.9)
    assert (n1[:, 9] == 1).all() and np.array_equal(bits(o1[:, 9]), bits(f1[:, 9]))
    assert (n1[:, :9] == 2).all() and (n1[:, 10:W_ - 1] == 2).all() and (n1[:, W_ - 1] == 1).all()
    # a pixel that is a miss now keeps length 0 whatever lies behind it in the history
    o2, _, n2, _ = temporal_model(st, f1, plane_gbuffer(prev, miss=miss), prev, 8, 0.25, 0.9)
    assert (n2[miss] == 0).all() and np.array_equal(bits(o2[miss]), bits(f1[miss]))


def test_model_half_pixel_step_blends_two_taps_and_takes_the_smaller_length():
    prev, cur = plane_camera(0), plane_camera(0.5)
    f0, f1 = frame_of(5), frame_of(6)
    _, _, _, st = temporal_model(None, f0, plane_gbuffer(prev), prev, 8, 0.25, 0.9)
    st["colour"][:, 12:, 3] = 4  # pretend the right half is older
    _, _, n, st1 = temporal_model(st, f1, plane_gbuffer(cur), cur, 8, 0.25, 0.9)
    assert (n[:, :11] == 2).all() and (n[:, 11] == 2).all() and (n[:, 12:W_ - 1] == 5).all()
    # the last column has one tap in the image, of weight 1/2: accepted (>= 1/64)
    assert (n[:, W_ - 1] == 5).all()
    L0, L1 = f0[..., :3] * f0[..., :3], f1[..., :3] * f1[..., :3]
    hc = (f32(0.5) * L0[:, 3] + f32(0.5) * L0[:, 4]) / f32(1)
    assert np.array_equal(st1["colour"][:, 3, :3], hc + (L1[:, 3] - hc) * f32(0.5))


# ---- synthetic inputs at the contract's edges: exact plane steps, an analytic room, a camera path, an injection table --------------------
# (tests/test_gpu_temporal_synthetic.py runs all of them through k_temporal; the tests below hold the model, and the generators, to account)
def _edge(W, H, which):
    return {"right": (slice(None), W - 1), "left": (slice(None), 0), "bottom": (H - 1, slice(None)), "top": (0, slice(None)),
            "corner": (H - 1, W - 1)}[which]


_B6, _B7 = 1.0 - 2.0 ** -6, 1.0 - 2.0 ** -7
_NEXT = float(np.nextafter(f32(-1), f32(0)))  # -(1 - 2^-24): the camera's pixel00 rounds it away, column 0 lands on sx == -1 exactly
# id: (shift in x, shift in y as handed to plane_camera, the shifts that reach sx and sy, the edge whose pixels keep ONE tap or none,
#      whether the contract accepts that edge). Everywhere else all weights of the taps in the image sum to a power of two >= 1/16: n = 2.
PLANE_STEPS = {
    "x+(1-2^-6)": (_B6, 0.0, _B6, 0.0, "right", True),      # one tap of weight exactly 1/64: Wsum == 1/64 passes
    "x+(1-2^-7)": (_B7, 0.0, _B7, 0.0, "right", False),     # 1/128
    "x-(1-2^-6)": (-_B6, 0.0, -_B6, 0.0, "left", True),     # sx = -1 + 2^-6, inside (-1, 0): tap (1, 0) of weight 1/64
    "x-(1-2^-7)": (-_B7, 0.0, -_B7, 0.0, "left", False),
    "x-1": (-1.0, 0.0, -1.0, 0.0, "left", False),           # sx == -1: step 3 fails
    "x-next(-1)": (_NEXT, 0.0, -1.0, 0.0, "left", False),
    "y+(1-2^-6)": (0.0, _B6, 0.0, _B6, "bottom", True),
    "y+(1-2^-7)": (0.0, _B7, 0.0, _B7, "bottom", False),
    "y-(1-2^-6)": (0.0, -_B6, 0.0, -_B6, "top", True),
    "y-(1-2^-7)": (0.0, -_B7, 0.0, -_B7, "top", False),
    "y-1": (0.0, -1.0, 0.0, -1.0, "top", False),
    "y-next(-1)": (0.0, _NEXT, 0.0, -1.0, "top", False),
    "corner 2^-3*2^-3": (0.875, 0.875, 0.875, 0.875, "corner", True),      # the weight is a product: 1/64
    "corner 2^-3*2^-4": (0.875, 0.9375, 0.875, 0.9375, "corner", False),   # 1/128
}
PLANE_SIZES = [(24, 10), (80, 10)]


def plane_step_inputs(case, W, H):
    """The two calls of a plane step: (camera, frame, G-buffer) of the first call and of the second."""
    kx, ky = PLANE_STEPS[case][:2]
    prev, cur = plane_camera(0, W, H), plane_camera(kx, W, H, ky)
    return (prev, frame_of(1, W, H), plane_gbuffer(prev)), (cur, frame_of(2, W, H), plane_gbuffer(cur))


def plane_step_by_hand(case, f0, f1):
    """(out_f32, history_len) of the second call, from the contract by hand: sx = x + kx and sy = y + ky exactly, the taps' weights are
    multiples of 2^-14, the squares of the frames multiples of 2^-10 below 4, every Wsum a power of two: float64 carries each step without a
    rounding, so the fp32 contract has to give these very values (asserted: they fit float32)."""
    _, _, kx, ky, which, accepted = PLANE_STEPS[case]
    H, W = f0.shape[:2]
    L0, L1 = f0[..., :3].astype(np.float64) ** 2, f1[..., :3].astype(np.float64) ** 2
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx, sy = xs + kx, ys + ky
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    S, wsum = np.zeros((H, W, 3)), np.zeros((H, W))
    for j in (0, 1):
        for i in (0, 1):
            tx, ty = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
            w = (fx if i else 1 - fx) * (fy if j else 1 - fy)
            use = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H) & (w > 0)
            S += np.where(use[..., None], w[..., None] * L0[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)], 0)
            wsum += np.where(use, w, 0)
    n = np.full((H, W), 2, f32)
    n[_edge(W, H, which)] = 2 if accepted else 1  # the hand-derived answer; the weights above must agree with it
    assert np.array_equal(wsum >= 1 / 64, n == 2) and (np.log2(wsum[wsum > 0]) % 1 == 0).all()
    with np.errstate(all="ignore"):
        Hc = S / wsum[..., None]
        Lb = Hc + (L1 - Hc) * 0.5
    Lb = np.where((n == 2)[..., None], Lb, 0)
    assert np.array_equal(Lb.astype(f32).astype(np.float64), Lb)
    out = np.ones((H, W, 4), f32)
    out[..., :3] = np.where((n == 2)[..., None], np.sqrt(Lb.astype(f32)), f1[..., :3])
    return out, n


@pytest.mark.parametrize("W,H", PLANE_SIZES)
@pytest.mark.parametrize("case", PLANE_STEPS)
def test_model_plane_steps_at_the_tap_weight_threshold_and_the_border_band(case, W, H):
    (c0, f0, g0), (c1, f1, g1) = plane_step_inputs(case, W, H)
    _, _, kx, ky, which, accepted = PLANE_STEPS[case]
    ok, sx, sy = reproject(c0, g1["prev_position"], W, H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    assert np.array_equal(sx.astype(np.float64), xs + kx) and np.array_equal(sy.astype(np.float64), ys + ky)  # exact
    if case.endswith("1") or "next" in case:
        assert not ok[_edge(W, H, which)].any() and np.delete(ok, 0, axis=1 if which == "left" else 0).all()  # sx == -1 fails step 3
    else:
        assert ok.all()
    _, _, _, st = temporal_model(None, f0, g0, c0, 8, 0.25, 0.9)
    o, u, n, st1 = temporal_model(st, f1, g1, c1, 8, 0.25, 0.9)
    want_o, want_n = plane_step_by_hand(case, f0, f1)
    assert np.array_equal(n, want_n)
    assert (n[_edge(W, H, which)] == (2 if accepted else 1)).all() and (n == 2).sum() >= W * H - max(W, H)
    assert np.array_equal(bits(o), bits(want_o))
    if not accepted:
        assert np.array_equal(bits(o[_edge(W, H, which)]), bits(f1[_edge(W, H, which)]))  # the input's own bits
    assert np.array_equal(u[..., :3], to_unorm8(want_o[..., :3]))


ROOM_LO, ROOM_HI = np.array([-2.0, -1.0, -3.0]), np.array([2.0, 1.5, 3.0])
ROOM_WINDOW = ((-0.8, 0.2), (0.0, 0.9))    # x and y range of the hole in the wall z = -3: a miss
ROOM_PANEL_X = 0.5                          # the part of that wall with x > 0.5 moved by ROOM_MOTION since the previous call
ROOM_MOTION = np.array([0.05, 0.0, 0.24])   # (its depth component just below the default sigma_position: the panel straddles the test)
ROOM_PARAMS = dict(max_history=32, sigma_position=0.25, cos_normal=0.9)


def room_gbuffer(cam, motion=ROOM_MOTION):
    """normal, position, prev_position of the inside of the box ROOM_LO .. ROOM_HI seen by `cam` (centre inside the box): every pixel's
    unjittered ray (rt_scene_gbuffer's pixel centre and direction, fp32) intersected with the walls in float64, rounded to fp32."""
    W, H = int(cam.width), int(cam.height)
    c, p00, du, dv = _cam_vectors(cam)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pc = (p00 + xs[..., None].astype(f32) * du) + ys[..., None].astype(f32) * dv
    d, c64 = (pc - c).astype(np.float64), c.astype(np.float64)
    with np.errstate(all="ignore"):
        tk = np.where(d != 0, (np.where(d > 0, ROOM_HI, ROOM_LO) - c64) / d, np.inf)
    k = np.argmin(tk, -1)
    t = np.take_along_axis(tk, k[..., None], -1)[..., 0]
    pos = c64 + d * t[..., None]
    dk = np.take_along_axis(d, k[..., None], -1)[..., 0]
    N = np.zeros((H, W, 4), f32)
    np.put_along_axis(N[..., :3], k[..., None], (-np.sign(dk)).astype(f32)[..., None], -1)
    back = (k == 2) & (dk < 0)
    (x_lo, x_hi), (y_lo, y_hi) = ROOM_WINDOW
    miss = back & (pos[..., 0] > x_lo) & (pos[..., 0] < x_hi) & (pos[..., 1] > y_lo) & (pos[..., 1] < y_hi)
    P = np.concatenate([pos, t[..., None]], -1).astype(f32)
    Q = P.copy()
    Q[..., 3] = 1
    panel = back & ~miss & (pos[..., 0] > ROOM_PANEL_X)
    Q[panel, :3] = (pos[panel] - motion).astype(f32)
    P[miss], N[miss], Q[miss] = (0, 0, 0, np.inf), 0, 0
    return {"normal": N, "position": P, "prev_position": Q}


def hand_camera(W, H, center, direction, focal, roll_deg=0.0, step=None):
    """An rt_camera filled by hand (float64, rounded once): rt_camera_init's camera turned by `roll_deg` about its view axis — delta_u and
    delta_v stay perpendicular, which is all the contract asks, and rt_camera_init cannot make it — with pixels `step` apart (None:
    rt_camera_init's 2 / H) at the same field of view."""
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    right = np.cross(d, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, d)
    a = np.deg2rad(roll_deg)
    r2, u2 = np.cos(a) * right + np.sin(a) * up, np.cos(a) * up - np.sin(a) * right
    step = 2.0 / H if step is None else float(step)
    du, dv = r2 * step, -u2 * step
    c = np.asarray(center, np.float64)
    p00 = c + d * (focal * step * H / 2) - (W / 2) * du - (H / 2) * dv
    cam = abi.rt_camera()
    cam.center[:], cam.pixel00[:], cam.delta_u[:], cam.delta_v[:] = c.tolist(), p00.tolist(), du.tolist(), dv.tolist()
    cam.width, cam.height = W, H
    return cam


def room_path(W, H):
    """[(tag, rt_camera)]: the camera of every call. Tags: "small" a step after which most of the image keeps its history, "same" the
    previous camera again, "turn180" / "turn90", "other" anything else (a roll, a zoom out)."""
    from rtamd.renderer import Camera

    def init(c, d, f):
        return Camera((W, H), c, d, f).c
    return [
        ("other", init((0, 0, 0), (0, 0, -1), 1.0)),
        ("small", init((0.05, 0.02, -0.03), (0.03, 0.01, -1), 1.0)),               # translation, yaw and pitch
        ("small", init((0.1, 0.03, -0.05), (0.06, -0.02, -1), 1.0)),
        ("same", init((0.1, 0.03, -0.05), (0.06, -0.02, -1), 1.0)),
        ("small", init((0.1, 0.03, -0.05), (0.06, -0.02, -1), 1.25)),              # zoom in
        ("small", init((0.08, 0.03, -0.04), (0.05, -0.01, -1), 1.1)),              # ... and out
        ("small", init((0, 0, 0), (0.05, 0, -1), 1.0)),                            # centre at the origin: the next call's "axis" row
        ("other", hand_camera(W, H, (0.02, 0.01, 0.0), (0.05, 0.0, -1), 1.0, roll_deg=20)),
        ("small", hand_camera(W, H, (0.04, 0.0, 0.02), (0.03, 0.01, -1), 1.0, roll_deg=21)),   # through a rolled previous camera
        ("small", hand_camera(W, H, (0.05, 0.0, 0.03), (0.02, 0.01, -1), 1.0, roll_deg=21, step=2.0)),  # |cross(du, dv)| = 4
        ("other", init((0.05, 0.0, 0.03), (0.02, 0.01, -1), 1.0)),                 # through it: the "far" row overflows to s = +0
        ("turn180", init((0.05, 0.0, 0.03), (-0.02, -0.01, 1), 1.0)),              # every point lies behind the previous camera
        ("small", init((0.03, 0.02, 0.0), (0.01, -0.02, 1), 1.0)),
        ("turn90", init((0, 0, 0), (1, 0.0, 0.15), 1.0)),                          # some behind it, some in front and off the window
        ("small", init((0.02, 0.01, 0.01), (1, 0.02, 0.12), 1.0)),
        ("same", init((0.02, 0.01, 0.01), (1, 0.02, 0.12), 1.0)),
        ("small", init((0.0, 0.0, 0.0), (1, 0.0, 0.1), 1.1)),
    ]


INJECT_ROWS = ("centre", "centre_plane", "behind", "nan", "inf", "axis", "far")


def injection_points(prev_cam):
    """row -> the point (3 float32) written into prev_position, from the previous camera's centre c' and m' = cross(du', dv'); a is the
    unit view axis. None: the row cannot be made with this camera ("axis" needs c' = 0, next to which 1e-30 survives)."""
    c, p00, du, dv = (v.astype(np.float64) for v in _cam_vectors(prev_cam))
    m = np.cross(du, dv)
    a = m / np.linalg.norm(m) * np.sign(np.dot(p00 - c, m))
    front = c + a * np.linalg.norm(p00 - c)
    rows = {
        "centre": c,                                          # dot(r, m') = 0: s = em / 0
        "centre_plane": c + 3 * du,                           # in the plane through c' (to rounding: a huge or an infinite s)
        "behind": c - a * np.linalg.norm(p00 - c) + 2 * du,   # s < 0
        "nan": np.array([np.nan, front[1], front[2]]),
        "inf": np.array([front[0], np.inf, front[2]]),        # r.y = inf: dot(r, m') is NaN (m'.y = 0) or infinite, s NaN or a zero
        "axis": 1e-30 * a if not c.any() else None,           # s ~ 1e30 |e|, finite: lands on the principal point
        "far": 3e38 * a,                                      # s ~ |e| / 3e38: subnormal; with |m'| = 4 dot(r, m') overflows and s = +0
    }
    return {k: None if v is None else v.astype(f32) for k, v in rows.items()}


def s_class(prev_cam, q):
    """The class of step 3's s for the point q, from float64 arithmetic on the fp32 inputs and the limits of binary32 (not from
    reproject): "nan", "inf", "zero", "negative", "subnormal" or "normal"."""
    c, p00, du, dv = (v.astype(np.float64) for v in _cam_vectors(prev_cam))
    m = np.cross(du, dv)
    fmax, fmin = float(np.finfo(f32).max), float(np.finfo(f32).tiny)
    with np.errstate(all="ignore"):
        den, num = np.dot(np.asarray(q, np.float64) - c, m), np.dot(p00 - c, m)
        if np.isnan(den):
            return "nan"
        if abs(den) > fmax:
            return "zero"
        s = np.inf if den == 0 else num / den
    if abs(s) > fmax:
        return "inf"
    return "negative" if s < 0 else "subnormal" if s < fmin else "normal"


def room_frame(call, W, H):
    """A frame with colours in [0, 1.5), one pixel in 16 exactly 0, a row around 1e-20 (squares subnormal) and a row around 1e19 (squares
    just finite). (Images of fewer than three rows: columns; a single pixel: by turns.)"""
    rng = np.random.default_rng(7919 * call + 31 * W + H)
    f = np.ones((H, W, 4), f32)
    rgb = rng.uniform(0.0, 1.5, (H, W, 3)).astype(f32)
    rgb[rng.integers(0, 16, (H, W)) == 0] = 0
    tiny, huge = (rng.uniform(0.5, 1.5, (H, W, 3)) * 1e-20).astype(f32), (rng.uniform(0.5, 1.5, (H, W, 3)) * 1e19).astype(f32)
    if H >= 3:
        rgb[H // 3], rgb[2 * H // 3] = tiny[H // 3], huge[2 * H // 3]
    elif W >= 3:
        rgb[:, W // 3], rgb[:, 2 * W // 3] = tiny[:, W // 3], huge[:, 2 * W // 3]
    elif call % 3:
        rgb[:] = tiny if call % 3 == 1 else huge
    f[..., :3] = rgb
    return f


def room_sequence(W, H, inject=True):
    """Yields (call, tag, camera, frame, G-buffer, {row: flat pixel indices}) along room_path, the injection table written over up to
    three hit pixels per row of every call after the first (of every second call on images of under 64 pixels, which would otherwise never
    keep a history)."""
    prev = None
    for call, (tag, cam) in enumerate(room_path(W, H)):
        g = room_gbuffer(cam)
        where = {}
        if inject and prev is not None and (W * H >= 64 or call % 2):
            pts = {k: v for k, v in injection_points(prev).items() if v is not None}
            rows = [r for r in INJECT_ROWS if r in pts]
            hits = np.flatnonzero(np.isfinite(g["position"][..., 3]).ravel())
            rng = np.random.default_rng(1000 + call)
            pick = rng.choice(hits, size=min(len(hits), 3 * len(rows)), replace=False)
            Q = g["prev_position"].reshape(-1, 4)
            for j, p in enumerate(pick):
                r = rows[(j + call) % len(rows)]
                Q[p, :3] = pts[r]
                where.setdefault(r, []).append(int(p))
        yield call, tag, cam, room_frame(call, W, H), g, where
        prev = cam


def test_room_is_a_closed_box_with_a_window_and_a_panel(rtlib):
    W, H = 97, 43
    cams = room_path(W, H)
    assert len(cams) >= 10
    g = room_gbuffer(cams[0][1])
    P, N, Q = g["position"], g["normal"], g["prev_position"]
    hit = np.isfinite(P[..., 3])
    assert 0.01 < (~hit).mean() < 0.2 and (P[~hit][:, :3] == 0).all() and (N[~hit] == 0).all() and (Q[~hit] == 0).all()
    assert (P[hit][:, 3] > 0).all() and (np.abs(N[hit][:, :3]).sum(-1) == 1).all() and (Q[hit][:, 3] == 1).all()
    on_wall = np.isclose(P[hit][:, :3], ROOM_LO, atol=1e-5) | np.isclose(P[hit][:, :3], ROOM_HI, atol=1e-5)
    assert (on_wall & (N[hit][:, :3] != 0)).any(-1).all()
    assert ((P[hit][:, :3] > ROOM_LO - 1e-5) & (P[hit][:, :3] < ROOM_HI + 1e-5)).all()
    moved = hit & (Q[..., :3] != P[..., :3]).any(-1)
    assert moved.any() and (P[moved][:, 0] > ROOM_PANEL_X).all() and np.allclose(P[moved][:, :3] - Q[moved][:, :3], ROOM_MOTION, atol=1e-6)
    assert len({N[hit][i, :3].tobytes() for i in range(hit.sum())}) >= 5  # five of the six walls are in view
    # the path holds what it must: two equal consecutive cameras, both zoom directions, a rolled and a coarse hand-filled camera
    raw = [bytes(c) for _, c in cams]
    assert any(a == b for a, b in zip(raw, raw[1:]))
    for _, c in cams:
        _, _, du, dv = _cam_vectors(c)
        assert abs(float(_dot3(du, dv))) <= 1e-6 * float(_dot3(du, du))  # perpendicular
    assert any(abs(float(_cam_vectors(c)[2][1])) > 0.1 * float(np.linalg.norm(_cam_vectors(c)[2])) for _, c in cams)   # rolled: du leaves the horizontal
    assert any(np.isclose(np.linalg.norm(_cross(*_cam_vectors(c)[2:])), 4.0) for _, c in cams)


def test_injection_rows_have_the_s_the_table_promises(rtlib):
    """The s of every row under every camera of the path as the previous camera: its class from float64 (s_class) and by hand."""
    W, H = 97, 43
    seen = set()
    for tag, cam in room_path(W, H):
        pts = injection_points(cam)
        coarse = bool(np.isclose(np.linalg.norm(_cross(*_cam_vectors(cam)[2:])), 4.0))
        for row, q in pts.items():
            if q is None:
                continue
            with np.errstate(all="ignore"):
                s = reproject_s(cam, q)
                ok, sx, sy = reproject(cam, q, W, H)
            if row == "centre_plane":  # decided by roundings under a general camera: never accepted, and exact on the plane camera below
                assert not ok or not (-1 < sx < W and -1 < sy < H)
                continue
            if row == "inf":  # inf * m'.y: NaN where the fp32 cross product's y is exactly 0 (a level camera), else an infinite dot and a zero s
                assert np.isnan(s) or s == 0, (tag, s)
                assert not ok
                seen.add((row, "nan" if np.isnan(s) else "zero"))
                continue
            cls = s_class(cam, q)
            want = {"centre": "inf", "behind": "negative", "nan": "nan", "axis": "normal", "far": "zero" if coarse else "subnormal"}[row]
            assert cls == want, (tag, row, cls)
            seen.add((row, cls))
            tiny = float(np.finfo(f32).tiny)
            assert {"nan": np.isnan(s), "inf": np.isinf(s), "zero": s == 0, "negative": np.isfinite(s) and s < 0,
                    "subnormal": 0 < s < tiny, "normal": np.isfinite(s) and s >= tiny}[cls], (tag, row, cls, s)
            if row == "axis":
                assert 1e29 < s < 1e31 and ok and abs(sx - W / 2) < 1 and abs(sy - H / 2) < 1  # on the principal point
            if row == "far":
                assert not np.signbit(s) and bool(ok) == (not coarse)  # +0 fails on s > 0; a subnormal s goes on to the window, and is in it
            if cls != "normal" and cls != "subnormal":
                assert not ok
    assert {("centre", "inf"), ("behind", "negative"), ("nan", "nan"), ("inf", "nan"), ("inf", "zero"), ("axis", "normal"),
            ("far", "subnormal"), ("far", "zero")} <= seen, seen
    cam = plane_camera(2)
    c = np.array(list(cam.center), f32)
    for k in (1, -3, 7):
        q = c + f32(k) * np.array(list(cam.delta_u), f32)
        with np.errstate(all="ignore"):
            assert np.isinf(reproject_s(cam, q)) and not reproject(cam, q, W_, H_)[0]  # r = (k/16, 0, 0), m = (0, 0, -2^-8): the dot is 0


def _reference_projection(prev_cam, Q):
    """(lam, sx, sy) float64 with c' + lam (Q - c') = p00' + sx du' + sy dv': a linear solve, not the contract's cross and dot products."""
    c, p00, du, dv = (v.astype(np.float64) for v in _cam_vectors(prev_cam))
    A = np.empty(Q.shape[:-1] + (3, 3))
    A[..., 0], A[..., 1], A[..., 2] = Q.astype(np.float64) - c, -du, -dv
    return np.moveaxis(np.linalg.solve(A, np.broadcast_to(p00 - c, Q.shape[:-1] + (3,))[..., None])[..., 0], -1, 0)


PROJECTION_UNITS = 4 * 7.8


@pytest.mark.parametrize("W,H", [(97, 43), (640, 360)])
def test_model_projection_against_a_float64_solve(rtlib, W, H):
    """reproject's fp32 sx, sy against _reference_projection for every hit of the room under every pair of consecutive cameras of the path
    (yawed, pitched, zoomed, rolled, coarse), where the reference lands in the window. Unit: 2^-24 |p00' - c'| / |du'|, about the rounding of
    one coordinate of h in pixel steps. Measured largest deviation: 7.72 units at 97 x 43 and 7.79 at 640 x 360 (0.0004 pixel); the bound is 4 times the larger, PROJECTION_UNITS, since
    a sample does not reach the worst rounding pattern. This pins the model to geometry; the kernel is not involved."""
    cams = [c for _, c in room_path(W, H)]
    worst, n = 0.0, 0
    for prev, cur in zip(cams, cams[1:]):
        g = room_gbuffer(cur)
        Q = g["prev_position"][np.isfinite(g["position"][..., 3])][:, :3]
        lam, rx, ry = _reference_projection(prev, Q)
        use = (lam > 0) & (rx > -1) & (rx < W) & (ry > -1) & (ry < H)
        if not use.any():
            continue
        ok, sx, sy = reproject(prev, Q, W, H)
        c, p00, du, _ = (v.astype(np.float64) for v in _cam_vectors(prev))
        unit = 2.0 ** -24 * np.linalg.norm(p00 - c) / np.linalg.norm(du)
        dev = max(np.abs(sx[use] - rx[use]).max(), np.abs(sy[use] - ry[use]).max()) / unit
        inner = use & (rx > -0.99) & (rx < W - 0.01) & (ry > -0.99) & (ry < H - 0.01)
        assert ok[inner].all()
        worst, n = max(worst, dev), n + int(use.sum())
    print(f"\nprojection {W}x{H}: largest deviation {worst:.2f} units over {n} points")
    assert n > 5 * W * H and worst <= PROJECTION_UNITS, worst


def test_model_running_mean_on_the_plane():
    """Static camera and scene, max_history >= k: the stored colour after k calls is the mean of the k linear frames. Per call the blend
    rounds four times (S / Wsum is exact here: one tap of weight 1): L - Hc, * a, + Hc, and a = 1 / n itself, each at most 2^-24 of max L
    relative to the values in play, so |stored - mean| <= 4 k 2^-24 max L. (Only on this camera: DESIGN.md §15.)"""
    cam = plane_camera(0)
    g = plane_gbuffer(cam)
    st, acc, k_max = None, np.zeros((H_, W_, 3)), 64
    for k in range(1, k_max + 1):
        f = frame_of(100 + k)
        acc += f[..., :3].astype(np.float64) ** 2
        _, _, n, st = temporal_model(st, f, g, cam, 4096, 0.25, 0.9)
        assert (n == k).all()
        err = np.abs(st["colour"][..., :3].astype(np.float64) - acc / k).max()
        assert err <= 4 * k * 2.0 ** -24 * (63 / 32) ** 2, (k, err)


def room_classes(W, H, params=ROOM_PARAMS):
    """Runs the model along room_sequence and classifies every hit pixel of every call after the first. Returns ({class: count},
    [(call, tag, blended fraction of the hits)])."""
    count, calls, st = {}, [], None

    def add(name, mask):
        count[name] = count.get(name, 0) + int(mask.sum())
    for call, tag, cam, frame, g, where in room_sequence(W, H):
        tr = {}
        _, _, n, st = temporal_model(st, frame, g, cam, trace=tr, **params)
        if not tr:
            continue
        hit, s, ok, good, taps = tr["hit"], tr["s"], tr["ok"], tr["good"], tr["taps"]
        calls.append((call, tag, float(good[hit].mean())))
        with np.errstate(all="ignore"):
            front = np.isfinite(s) & (s > 0)
            add("s <= 0", hit & (s <= 0))
            add("s == +0", hit & (s == 0) & ~np.signbit(s))
            add("s not finite", hit & ~np.isfinite(s))
            add("s subnormal", hit & (s > 0) & (s < np.finfo(f32).tiny))
            add("off-window", hit & front & ~ok)
        sx, sy, fx, fy = tr["sx"], tr["sy"], tr["fx"], tr["fy"]
        add("accepted with sx < 0 or sy < 0", good & ((sx < 0) | (sy < 0)))
        add("accepted with sx > W - 1 or sy > H - 1", good & ((sx > W - 1) | (sy > H - 1)))
        add("fx == 0 and fy == 0", ok & (fx == 0) & (fy == 0))
        base = [ok & t["inside"] & (t["w"] > 0) & t["hit"] for t in taps]
        w64 = [t["w"].astype(np.float64) for t in taps]
        wsum = lambda masks: sum(np.where(m, w, 0) for m, w in zip(masks, w64))
        w_all = wsum([t["valid"] for t in taps])
        w_nopos = wsum([b & t["nrm_ok"] for b, t in zip(base, taps)])
        w_nonrm = wsum([b & t["pos_ok"] for b, t in zip(base, taps)])
        add("rejected by Wsum < 1/64 alone", ok & (w_all > 0) & (w_all < 1 / 64) & (wsum(base) == w_all))
        add("rejected by the position test alone", ok & (w_all < 1 / 64) & (w_nopos >= 1 / 64) & (w_nonrm < 1 / 64))
        add("rejected by the normal test alone", ok & (w_all < 1 / 64) & (w_nonrm >= 1 / 64) & (w_nopos < 1 / 64))
        n_valid = sum(t["valid"].astype(int) for t in taps)
        for k in (1, 2, 3, 4):
            add(f"accepted with {k} valid taps", good & (n_valid == k))
        n_lo = np.minimum.reduce([np.where(t["valid"], t["n"], np.inf) for t in taps])
        n_hi = np.maximum.reduce([np.where(t["valid"], t["n"], -np.inf) for t in taps])
        add("accepted with taps of different lengths", good & (n_hi > n_lo))
        shorter = [ok & t["inside"] & (t["w"] == 0) & t["hit"] & t["pos_ok"] & t["nrm_ok"] & (t["n"] < n_lo) for t in taps]
        add("a zero-weight tap holds a shorter history", good & ((fx == 0) | (fy == 0)) & np.logical_or.reduce(shorter))
        for row, px in where.items():
            add(f"injected {row} blended", good.ravel()[px])
    return count, calls


ROOM_CLASSES = ["s <= 0", "s == +0", "s not finite", "s subnormal", "off-window", "accepted with sx < 0 or sy < 0",
                "accepted with sx > W - 1 or sy > H - 1", "fx == 0 and fy == 0", "rejected by Wsum < 1/64 alone",
                "rejected by the position test alone", "rejected by the normal test alone", "accepted with 1 valid taps",
                "accepted with 2 valid taps", "accepted with 3 valid taps", "accepted with 4 valid taps",
                "accepted with taps of different lengths", "a zero-weight tap holds a shorter history"]


def test_room_path_reaches_every_rule(rtlib):
    """The conditions under which the GPU comparison on the room means something, on the model alone (97 x 43, the defaults of the GPU
    test): every class of ROOM_CLASSES occurs somewhere along the path, most of the image is blended after every small step, nothing after
    the half turn; and with both guide tests off the rows that land on the principal point (a subnormal s, s ~ 1e30) ARE blended, so that a
    kernel that flushes s to zero differs from the model."""
    count, calls = room_classes(97, 43)
    print("\n" + "\n".join(f"{k}: {v}" for k, v in count.items()) + "\n" + " ".join(f"{c}:{t}:{f:.2f}" for c, t, f in calls))
    for name in ROOM_CLASSES:
        assert count.get(name, 0) > 0, name
    assert len(calls) >= 10
    for call, tag, frac in calls:
        if tag in ("small", "same"):
            assert frac >= 0.5, (call, tag, frac)
        if tag == "turn180":
            assert frac == 0, (call, frac)
    assert {t for _, t, _ in calls} >= {"small", "same", "turn180", "turn90", "other"}
    open_count, _ = room_classes(97, 43, dict(max_history=32, sigma_position=INF, cos_normal=-1.0))
    assert open_count["injected far blended"] > 0 and open_count["injected axis blended"] > 0, open_count


# ---- listings and the CLI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit,kernel", [("rt_gbuffer.hip", "k_gbuffer"), ("rt_gbuffer_motion.hip", "k_gbuffer_motion")])
def test_gbuffer_kernels_pass_the_isa_hazard_scan(tmp_path, unit, kernel):
    from test_isa_hazards import _check
    groups = _check(_listing(unit, tmp_path))
    assert any(kernel in k for k in groups), groups


def test_temporal_unit_passes_the_isa_hazard_scan_and_uses_plain_vector_memory(tmp_path):
    """rt_temporal.hip through the same checker (it has no traversal: no asm fetch may appear), and what the contract says of k_temporal: no
    atomics, no scratch, 16-byte loads and stores."""
    from test_isa_hazards import _check
    lines = _listing("rt_temporal.hip", tmp_path)
    assert _check(lines) == {}
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_ZN\w*k_temporal\w*:", ln))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = [ln.split(";")[0].strip() for ln in lines[start:end]]
    assert not any("atomic" in ln for ln in body)
    assert not any(ln.startswith("scratch_") for ln in body)
    wide = sum(bool(re.match(r"global_load_dwordx[34]\b", ln)) for ln in body)  # (x3 where the compiler sees that .w is not used)
    assert wide == 16, wide  # 4 inputs + 4 taps x 3 planes, each exactly once: nothing is fetched twice
    assert sum(ln.startswith("global_store_dwordx4") for ln in body) >= 4
    meta = "\n".join(lines[end:])
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta)


def _cli(*args):
    if not EXE.exists():
        import __graft_entry__ as g
        g.build()
    return subprocess.run([str(EXE), *args], capture_output=True, text=True, timeout=60)


def test_cli_refuses_temporal_without_an_animation_or_over_several_devices(rtlib):
    p = _cli("--temporal", "8", "cube.glb")
    assert p.returncode == 105 and "--temporal" in p.stderr and "--frames" in p.stderr
    p = _cli("--temporal", "8", "--frames", "1", "cube.glb")
    assert p.returncode == 105 and "--temporal" in p.stderr
    p = _cli("--temporal", "8", "--frames", "4", "--devices", "0,1", "cube.glb")
    assert p.returncode == 105 and "--temporal" in p.stderr and "one device" in p.stderr
    p = _cli("--temporal", "4097", "--frames", "4", "cube.glb")
    assert p.returncode == 105 and "--temporal" in p.stderr
    p = _cli("--help")
    assert p.returncode == 0 and "--temporal" in p.stdout
