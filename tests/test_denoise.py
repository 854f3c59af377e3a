"""CPU tests of the primary-hit G-buffer (rt_scene_gbuffer[_device]) and the a-trous denoiser (rt_denoiser_*, rt_denoise[_device]), and the
numpy float32 models that tests/test_gpu_denoise.py pins the device to bit for bit:

    gbuffer_model   a G-buffer from rt_intersect_batch's hits of the same rays and the scene description's arrays
    denoise_model   the filter of include/rt_mi355x.h (rt_denoise), with exp_m (csrc/denoise_math.h) restated op for op

Every numpy operation below is one IEEE binary32 operation on float32 arrays, in the order the contract states (no FMA in numpy)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "sycl-ray-tracer_amd" / "csrc"
EXE = REPO / "sycl-ray-tracer_amd" / "host" / "build" / "raytracer"
f32 = np.float32

# ---- exp_m (csrc/denoise_math.h) -------------------------------------------------------------------------------------------------------
EXP_CUTOFF = f32(-87.0)
LOG2E = f32(1.44269504088896341)
LN2_HI = f32(0.693145751953125)
LN2_LO = f32(1.42860676533018690e-06)
EXP_COEF = [f32(1) / f32(5040), f32(1) / f32(720), f32(1) / f32(120), f32(1) / f32(24), f32(1) / f32(6), f32(0.5), f32(1), f32(1)]


def exp_m(x):
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        n = np.rint(x * LOG2E)
        r = (x - n * LN2_HI) - n * LN2_LO
        p = np.full_like(x, EXP_COEF[0])
        for c in EXP_COEF[1:]:
            p = p * r + c
        e = np.clip(np.nan_to_num(n, nan=0.0).astype(np.int64), -126, 127)
        y = p * ((e + 127).astype(np.uint32) << np.uint32(23)).view(f32)
    return np.where(x >= EXP_CUTOFF, y, f32(0)).astype(f32)


# ---- the G-buffer ----------------------------------------------------------------------------------------------------------------------
def camera_rays(cam):
    """(org, d) of rt_scene_gbuffer's rays, (H*W, 3) each, row 0 first: pc = (pixel00 + x du) + y dv, d = pc - center."""
    w, h = int(cam.width), int(cam.height)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xs, ys = xs.reshape(-1).astype(f32), ys.reshape(-1).astype(f32)
    p00, du, dv, ce = (np.array(list(v), f32) for v in (cam.pixel00, cam.delta_u, cam.delta_v, cam.center))
    pc = (p00[None, :] + xs[:, None] * du[None, :]) + ys[:, None] * dv[None, :]
    d = pc - ce[None, :]
    return np.broadcast_to(ce, d.shape).copy(), d


def _normalize3(a):
    dot = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    inv = f32(1) / np.sqrt(dot)
    return a * inv[:, None]


def gbuffer_model(sd, cam, t, u, v, tri):
    """The G-buffer of `cam` over the scene description `sd`, given rt_intersect_batch's (t, u, v, tri) for camera_rays(cam)."""
    w, h = int(cam.width), int(cam.height)
    org, d = camera_rays(cam)
    n = w * h
    alb, nrm, pos = (np.zeros((n, 4), f32) for _ in range(3))
    miss = tri == 0xFFFFFFFF
    alb[miss, :3] = np.asarray(sd.sky, f32)
    pos[miss, 3] = np.inf
    hit = ~miss
    if hit.any():
        T = tri[hit].astype(np.int64)
        bx, by, th = u[hit].astype(f32), v[hit].astype(f32), t[hit].astype(f32)
        idx = np.asarray(sd.indices, np.int64).reshape(-1, 3)[T]
        nv, uv = np.asarray(sd.normals, f32).reshape(-1, 3), np.asarray(sd.uvs, f32).reshape(-1, 2)
        n0, n1, n2 = nv[idx[:, 0]], nv[idx[:, 1]], nv[idx[:, 2]]
        uv0, uv1, uv2 = uv[idx[:, 0]], uv[idx[:, 1]], uv[idx[:, 2]]
        inst = np.asarray(sd.tri_instance, np.int64)[T]
        wb = (f32(1) - bx) - by
        tu = (wb * uv0[:, 0] + bx * uv1[:, 0]) + by * uv2[:, 0]
        tv = (wb * uv0[:, 1] + bx * uv1[:, 1]) + by * uv2[:, 1]
        vn = _normalize3((wb[:, None] * n0 + bx[:, None] * n1) + by[:, None] * n2)
        nm = np.asarray(sd.normal_mats, f32).reshape(-1, 9)[inst]
        g = np.stack([(nm[:, 0] * vn[:, 0] + nm[:, 3] * vn[:, 1]) + nm[:, 6] * vn[:, 2],
                      (nm[:, 1] * vn[:, 0] + nm[:, 4] * vn[:, 1]) + nm[:, 7] * vn[:, 2],
                      (nm[:, 2] * vn[:, 0] + nm[:, 5] * vn[:, 1]) + nm[:, 8] * vn[:, 2]], 1)
        normal = _normalize3(g)
        mat_of = np.asarray(sd.inst_material, np.int64)[inst]
        a = np.zeros((T.shape[0], 3), f32)
        for mi, m in enumerate(sd.materials):
            sel = mat_of == mi
            if not sel.any():
                continue
            if m.type in (abi.RT_MAT_DIFFUSE, abi.RT_MAT_METALLIC):
                if m.tex_layer is None:
                    a[sel] = np.array([f32(c) for c in m.color], f32)
                else:
                    fu, fv = tu[sel] - np.floor(tu[sel]), tv[sel] - np.floor(tv[sel])
                    iu = np.clip(np.floor(fu * f32(512)).astype(np.int64), 0, 511)
                    iv = np.clip(np.floor(fv * f32(512)).astype(np.int64), 0, 511)
                    texel = np.asarray(sd.textures)[int(m.tex_layer), iv, iu, :3]
                    a[sel] = texel.astype(f32) / f32(255)
            elif m.type == abi.RT_MAT_DIELECTRIC:
                a[sel] = f32(1)
        alb[hit, :3] = a
        nrm[hit, :3] = normal
        o, dd = org[hit], d[hit]
        pos[hit, :3] = o + dd * th[:, None]
        pos[hit, 3] = th
    return {k: x.reshape(h, w, 4) for k, x in (("albedo", alb), ("normal", nrm), ("position", pos))}


# ---- the filter ------------------------------------------------------------------------------------------------------------------------
TAP_H = [f32(1) / f32(16), f32(0.25), f32(0.375), f32(0.25), f32(1) / f32(16)]


def coefficient(sigma):
    sigma = f32(sigma)
    if np.isinf(sigma):
        return f32(0)
    return f32(1) / (sigma * sigma)


def to_unorm8(c):
    return np.rint(np.fmin(np.fmax(c, f32(0)), f32(1)) * f32(255)).astype(np.uint8)


def _dot(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise_model(frame, gbuf, iterations, sigma_color, sigma_normal, sigma_position, sigma_albedo):
    """(f32 (H, W, 4), u8 (H, W, 4)) of rt_denoise on `frame` (H, W, 4 float32: sqrt(mean), alpha 1) with the guides `gbuf`."""
    frame = np.asarray(frame, f32)
    H, W = frame.shape[:2]
    if iterations == 0:
        u8 = np.concatenate([to_unorm8(frame[..., :3]), np.full((H, W, 1), 255, np.uint8)], -1)
        return frame.copy(), u8
    A, N, P = (np.asarray(gbuf[k], f32) for k in ("albedo", "normal", "position"))
    kc, kn, kx, ka = (coefficient(s) for s in (sigma_color, sigma_normal, sigma_position, sigma_albedo))
    L = frame[..., :3] * frame[..., :3]
    hit = np.isfinite(P[..., 3])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            kci, kni = f32(np.ldexp(kc, 2 * i)), f32(np.ldexp(kn, -2 * i))
            S = np.zeros((H, W, 3), f32)
            wsum = np.zeros((H, W), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    use = inside & (hit[qy, qx] == hit)
                    Lq = L[qy, qx]
                    E = np.zeros((H, W), f32)
                    if kci != 0:
                        E = E + _dot(L - Lq) * kci
                    if kni != 0:
                        E = E + _dot(N - N[qy, qx]) * kni
                    if kx != 0:
                        E = E + _dot(P[..., :3] - P[qy, qx, :3]) * kx
                    if ka != 0:
                        E = E + _dot(A - A[qy, qx]) * ka
                    w = (TAP_H[dy + 2] * TAP_H[dx + 2]) * exp_m(-E)
                    S = np.where(use[..., None], S + w[..., None] * Lq, S)
                    wsum = np.where(use, wsum + w, wsum)
            L = S / wsum[..., None]
    out = np.concatenate([np.sqrt(L), np.ones((H, W, 1), f32)], -1).astype(f32)
    u8 = np.concatenate([to_unorm8(out[..., :3]), np.full((H, W, 1), 255, np.uint8)], -1)
    return out, u8


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
NEW = ["rt_scene_gbuffer", "rt_scene_gbuffer_device", "rt_denoiser_create", "rt_denoiser_destroy", "rt_denoise", "rt_denoise_device"]


def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib):
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
        assert name in abi.PROTOTYPES, name
        assert hasattr(rtlib, name) and hasattr(devlib, name), name
    assert "typedef struct rt_denoise_params" in header
    assert C.sizeof(abi.rt_denoise_params) == 20
    assert [f[0] for f in abi.rt_denoise_params._fields_] == ["iterations", "sigma_color", "sigma_normal", "sigma_position", "sigma_albedo"]


def test_null_handles_and_bad_sizes_are_refused_without_a_device(rtlib):
    p = abi.rt_denoise_params(1, 1.0, 1.0, 1.0, 1.0)
    buf = np.zeros(16, np.float32)
    ptr = abi.fptr(buf)
    out = C.c_void_p()
    assert rtlib.rt_denoiser_create(-1, 4, 4, C.byref(out)) == abi.RT_ERR_INVALID and not out.value
    assert rtlib.rt_denoiser_create(0, 0, 4, C.byref(out)) == abi.RT_ERR_INVALID
    assert rtlib.rt_denoiser_create(0, 4, -1, C.byref(out)) == abi.RT_ERR_INVALID
    assert rtlib.rt_denoiser_create(0, 4, 4, None) == abi.RT_ERR_INVALID
    assert rtlib.rt_denoiser_create(0, 65536, 32768, C.byref(out)) == abi.RT_ERR_INVALID  # W * H = 2^31
    assert rtlib.rt_denoiser_create(0, 1, 2**31 - 1, C.byref(out)) == abi.RT_ERR_INVALID  # the filter's 1-D grid would pass 2^32 threads
    assert rtlib.rt_denoiser_create(0, 2**31 - 1, 1, C.byref(out)) == abi.RT_ERR_INVALID
    assert rtlib.rt_denoise(None, C.byref(p), ptr, ptr, ptr, ptr, ptr, None) == abi.RT_ERR_INVALID
    assert rtlib.rt_denoise_device(None, C.byref(p), 1, 1, 1, 1, 1, None, None) == abi.RT_ERR_INVALID
    cam = abi.rt_camera()
    cam.width, cam.height = 2, 2
    assert rtlib.rt_scene_gbuffer(None, C.byref(cam), ptr, ptr, ptr) == abi.RT_ERR_INVALID
    assert rtlib.rt_scene_gbuffer_device(None, C.byref(cam), 1, 1, 1, None) == abi.RT_ERR_INVALID
    rtlib.rt_denoiser_destroy(None)


def test_gbuffer_of_a_host_only_scene_is_refused(rtlib, scene_cache):
    from rtamd.renderer import Camera, Scene
    sd = scene_cache("cube")
    s = Scene(sd, device=-1)
    cam = Camera.for_scene(sd, (4, 3))
    with pytest.raises(abi.RtError) as e:
        s.gbuffer(cam)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    s.close()


def test_exp_m_is_within_4_ulp_of_exp():
    xs = np.concatenate([np.linspace(-87.0, 0.0, 4_000_001).astype(f32), -np.logspace(-45, 1.9, 100_000).astype(f32),
                         np.array([-87.0, -86.99999, -1e-30, -0.0], f32)])
    xs = xs[(xs >= -87.0) & (xs <= 0.0)]
    y = exp_m(xs).astype(np.float64)
    ref = np.exp(xs.astype(np.float64))
    ulp = np.spacing(ref.astype(f32)).astype(np.float64)
    assert (np.abs(y - ref) / ulp).max() <= 4.0
    assert exp_m(f32(-0.0)) == f32(1) and exp_m(f32(0.0)) == f32(1)
    assert exp_m(np.array([-87.01, -100.0, -np.inf, np.nan], f32)).tolist() == [0.0, 0.0, 0.0, 0.0]


def test_denoise_model_properties():
    """The model's own invariants: 0 iterations copy; a constant image stays constant; sigma = +inf equals the guide zeroed."""
    rng = np.random.default_rng(3)
    H, W = 9, 13
    frame = np.concatenate([rng.random((H, W, 3), dtype=f32) * f32(2), np.ones((H, W, 1), f32)], -1)
    g = {k: rng.random((H, W, 4), dtype=f32) for k in ("albedo", "normal", "position")}
    g["position"][2:4, 3:7, 3] = np.inf
    f0, b0 = denoise_model(frame, g, 0, 1, 1, 1, 1)
    assert np.array_equal(f0.view(np.uint32), frame.view(np.uint32)) and (b0[..., 3] == 255).all()
    c = np.full((H, W, 4), f32(0.5))
    c[..., 3] = 1
    fc, _ = denoise_model(c, g, 3, 0.5, 0.5, 0.5, 0.5)
    assert np.allclose(fc[..., :3], 0.5, rtol=2e-7)
    a, _ = denoise_model(frame, g, 2, 0.7, np.inf, 0.3, 0.2)
    gz = dict(g, normal=np.zeros_like(g["normal"]))
    b, _ = denoise_model(frame, gz, 2, 0.7, 0.001, 0.3, 0.2)
    assert np.array_equal(a, b)  # a zeroed guide contributes exact zeros whatever its sigma
    b2, _ = denoise_model(frame, gz, 2, 0.7, np.inf, 0.3, 0.2)
    assert np.array_equal(a, b2)


def _listing(unit, tmp_path):
    common = flags = None
    for line in (CSRC / "Makefile").read_text().splitlines():  # the product's own flags, read as tests/test_isa_hazards.py reads them
        if line.startswith("COMMON :="):
            common = line.split(":=", 1)[1].strip()
        if line.startswith("HIPFLAGS :="):
            flags = line.split(":=", 1)[1].strip().rstrip("\\").strip()
        elif flags is not None and flags.endswith("-fno-gpu-flush-denormals-to-zero") and "-mllvm" in line:
            flags += " " + line.strip()
    flags = flags.replace("$(COMMON)", common).replace("$(ARCH)", "gfx950")
    out = tmp_path / "unit.s"
    subprocess.run(["/opt/rocm/bin/hipcc", *flags.split(), "-S", "--cuda-device-only", str(CSRC / unit), "-o", str(out)], check=True,
                   capture_output=True, cwd=CSRC)
    return out.read_text().splitlines()


def test_gbuffer_kernel_passes_the_isa_hazard_scan(tmp_path):
    """k_gbuffer's unit (rt_gbuffer.hip) through tests/test_isa_hazards.py's checker: its asm node fetches are found, no rule is broken."""
    from test_isa_hazards import _check
    groups = _check(_listing("rt_gbuffer.hip", tmp_path))
    assert any("k_gbuffer" in k for k in groups), groups


def test_cli_refuses_more_than_ten_iterations(rtlib):
    if not EXE.exists():
        import __graft_entry__ as g
        g.build()
    p = subprocess.run([str(EXE), "--denoise", "11", "cube.glb"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--denoise" in p.stderr
    p = subprocess.run([str(EXE), "--help"], capture_output=True, text=True, timeout=60)
    assert "--denoise" in p.stdout
