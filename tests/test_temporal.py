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
    """(T, 3, 3) float32: every triangle's world-space vertices as the library computes them (scene_build.cpp, rt_update.hip:
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


def temporal_model(state, frame, gbuf, cam, max_history, sigma_position, cos_normal):
    """One call of rt_temporal_accumulate. `state`: None (no previous call since create / reset) or what the previous call returned.
    Returns (out_f32 (H, W, 4), out_u8 (H, W, 4), history_len (H, W), new state)."""
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
            for j in (0, 1):
                for i in (0, 1):
                    tx, ty = x0 + i, y0 + j
                    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                    tx, ty = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    w = (fx if i else gx) * (fy if j else gy)
                    Ct = state["colour"][ty, tx]
                    valid = ok & inside & (w > 0) & (Ct[..., 3] >= 1)
                    if kx != 0:
                        d = state["position"][ty, tx, :3] - Q[..., :3]
                        valid = valid & (_dot3(d, d) * kx <= f32(1))
                    if f32(cos_normal) != f32(-1):
                        valid = valid & (_dot3(N, state["normal"][ty, tx]) >= f32(cos_normal))
                    wsum = np.where(valid, wsum + w, wsum)
                    S = np.where(valid[..., None], S + w[..., None] * Ct[..., :3], S)
                    n_min = np.where(valid, np.fmin(n_min, Ct[..., 3]), n_min)
            n_next = np.fmin(n_min + f32(1), f32(max_history))
            good = ok & (wsum >= f32(1) / f32(64)) & (n_next != 1)
            Hc = S / wsum[..., None]
            a = f32(1) / n_next
            Lb = Hc + (L - Hc) * a[..., None]
        Lo = np.where(good[..., None], Lb, L).astype(f32)
        n_new = np.where(good, n_next, n_new).astype(f32)
        blended = good
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


def plane_camera(shift_px):
    """A camera looking down -z at the plane z = -1 (its own image plane, so P = the pixel centre and t = 1), moved sideways by `shift_px`
    pixel steps. du, dv are powers of two and every coordinate a small multiple of them: the model's arithmetic is exact."""
    cam = abi.rt_camera()
    cx = float(shift_px) * float(DU)
    cam.center[:] = [cx, 0.0, 0.0]
    cam.pixel00[:] = [cx - (W_ / 2) * float(DU), (H_ / 2) * float(DV), -1.0]
    cam.delta_u[:] = [float(DU), 0.0, 0.0]
    cam.delta_v[:] = [0.0, -float(DV), 0.0]
    cam.width, cam.height = W_, H_
    return cam


def plane_gbuffer(cam, miss=None, n_flip=None):
    ys, xs = np.meshgrid(np.arange(H_), np.arange(W_), indexing="ij")
    P = np.zeros((H_, W_, 4), f32)
    P[..., 0] = f32(cam.pixel00[0]) + xs.astype(f32) * DU
    P[..., 1] = f32(cam.pixel00[1]) - ys.astype(f32) * DV
    P[..., 2] = -1
    P[..., 3] = 1
    N = np.zeros((H_, W_, 4), f32)
    N[..., 2] = 1
    Q = P.copy()
    if n_flip is not None:
        N[:, n_flip, :3] = (1, 0, 0)
    if miss is not None:
        P[miss] = (0, 0, 0, np.inf)
        N[miss] = 0
        Q[miss] = 0
    return {"normal": N, "position": P, "prev_position": Q}


def frame_of(seed):
    rng = np.random.default_rng(seed)
    f = np.ones((H_, W_, 4), f32)
    f[..., :3] = rng.integers(0, 64, (H_, W_, 3)).astype(f32) / f32(32)  # multiples of 1/32 in [0, 2): squares are exact
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
