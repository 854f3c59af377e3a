"""Irradiance probe volumes (include/rt_mi355x.h: rt_probe_volume_*) without a GPU: the numpy model of the contract's steps 1, 2, 4, 5 and 6
that tests/test_gpu_probe_volume.py compares the device with (sphere_dir_model, entries_model, project_model, sample_model, and bake_model,
the whole bake around a path tracer handed in), what the model itself must show (unit directions that are uniform, a state that exhausts the
eight tries, the constant and the linear table, the empty scene through the CPU oracle), and the library in front of the device: the
exported symbols, the struct layouts, the refusals in their order, the wrappers' shape checks. The refusals that need a volume (dirs,
max_depth, sample before a table) cannot be reached without a device: tests/test_gpu_probe_volume.py has them."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd.renderer import ProbeVolume, Scene
from test_lightmap import entry_states
from test_path_query import xorshift_model

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
NONE = 0xFFFFFFFF
SYMBOLS = ["rt_probe_volume_create", "rt_probe_volume_destroy", "rt_probe_volume_entries", "rt_probe_volume_entries_device",
           "rt_probe_volume_bake", "rt_probe_volume_bake_device", "rt_probe_volume_set_sh", "rt_probe_volume_set_sh_device",
           "rt_probe_volume_get_sh", "rt_probe_volume_get_sh_device", "rt_probe_volume_sample", "rt_probe_volume_sample_device"]
TRIES = 8
BAND = np.array([1.0] + [0.6666667] * 3 + [0.25] * 5, f32)
SPHERE = f32(12.566371)  # step 4's weight is SPHERE / dirs


# ---- the model both files share ---------------------------------------------------------------------------------------------------------
def sphere_dir_model(state):
    """Step 2 on an array of states: (d (n, 3) float32, the states after the draws, fallback (n,) bool: all eight tries were rejected)"""
    a = np.array(state, np.uint32, copy=True).reshape(-1)
    n = len(a)
    x1, x2, s = np.zeros(n, f32), np.zeros(n, f32), np.full(n, 2.0, f32)
    done = np.zeros(n, bool)
    for _ in range(TRIES):
        u1, a1 = xorshift_model(a)
        u2, a2 = xorshift_model(a1)
        y1, y2 = f32(-1.0) + f32(2.0) * u1, f32(-1.0) + f32(2.0) * u2
        t = y1 * y1 + y2 * y2
        live = ~done
        x1, x2, s, a = np.where(live, y1, x1), np.where(live, y2, x2), np.where(live, t, s), np.where(live, a2, a)
        done = done | (live & (t < f32(1.0)))
    fb = ~done
    z1, z2 = x1 * f32(0.70710677), x2 * f32(0.70710677)
    x1, x2 = np.where(fb, z1, x1), np.where(fb, z2, x2)
    s = np.where(fb, x1 * x1 + x2 * x2, s)
    r = np.sqrt(f32(1.0) - s)
    d = np.stack([(f32(2.0) * x1) * r, (f32(2.0) * x2) * r, f32(1.0) - f32(2.0) * s], 1)
    assert d.dtype == f32 and a.dtype == np.uint32
    return d, a, fb


def probe_positions(origin, spacing, count):
    """(probes, 3) float32: origin + (float)index * spacing, probe p = (iz * count[1] + iy) * count[0] + ix"""
    origin, spacing = np.asarray(origin, f32), np.asarray(spacing, f32)
    iz, iy, ix = np.meshgrid(np.arange(count[2]), np.arange(count[1]), np.arange(count[0]), indexing="ij")
    idx = np.stack([ix, iy, iz], -1).reshape(-1, 3).astype(f32)
    pos = origin[None, :] + idx * spacing[None, :]
    assert pos.dtype == f32
    return pos


def entries_model(origin, spacing, count, dirs, seed):
    """Steps 1 and 2: {"pos", "dir": (probes * dirs, 3) float32, "state": (probes * dirs,) uint32, the path states, "fallback": bool}"""
    pos = np.repeat(probe_positions(origin, spacing, count), dirs, 0)
    d, a, fb = sphere_dir_model(entry_states(len(pos) // dirs, dirs, seed))
    return {"pos": pos, "dir": d, "state": a, "fallback": fb}


def Y_model(k, x, y, z):
    """Y_k on float32 arrays, the contract's bracketing"""
    if k == 0:
        return np.full(np.shape(x), 0.2820948, f32)
    if k in (1, 2, 3):
        return f32(0.48860252) * (y, z, x)[k - 1]
    if k in (4, 5, 7):
        a, b = {4: (x, y), 5: (y, z), 7: (x, z)}[k]
        return f32(1.0925485) * (a * b)
    if k == 6:
        return f32(0.31539157) * (f32(3.0) * (z * z) - f32(1.0))
    return f32(0.54627424) * (x * x - y * y)


def project_model(d, radiance, rays, probes, dirs):
    """Steps 4 and 5 from the path query's outputs over the probes * dirs entries (rays == NONE: rejected) -> (sh (probes, 9, 4), stats)"""
    d, rad = np.asarray(d, f32).reshape(probes, dirs, 3), np.asarray(radiance, f32).reshape(probes, dirs, 3)
    rays = np.asarray(rays, np.uint32).reshape(probes, dirs)
    valid = rays[:, 0] != NONE
    sh = np.zeros((probes, 9, 4), f32)
    w = SPHERE / f32(dirs)
    with np.errstate(all="ignore"):
        for k in range(9):
            c = np.zeros((probes, 3), f32)
            for j in range(dirs):
                c = c + rad[:, j] * Y_model(k, d[:, j, 0], d[:, j, 1], d[:, j, 2])[:, None]
            sh[:, k, :3] = c * w
    sh[~valid] = 0.0
    sh[valid, 0, 3] = 1.0
    assert sh.dtype == f32
    return sh, {"probes": probes, "valid": int(valid.sum()), "rays": int(rays[valid].astype(np.uint64).sum())}


def _axis(q, origin, spacing, count):
    with np.errstate(all="ignore"):
        g = (q - f32(origin)) / f32(spacing)
        g = np.fmin(np.fmax(g, f32(0.0)), f32(count - 1))
    i0 = np.zeros(len(q), np.int64) if count == 1 else np.minimum(g.astype(np.int64), count - 2)
    f = g - i0.astype(f32)
    return i0, f32(1.0) - f, f


def sample_model(origin, spacing, count, sh, pos, nrm):
    """Step 6: (n, 3) float32"""
    pos, nrm, sh = np.asarray(pos, f32), np.asarray(nrm, f32), np.asarray(sh, f32).reshape(-1, 9, 4)
    n = len(pos)
    fin = np.isfinite(pos).all(1) & np.isfinite(nrm).all(1)
    q = np.where(fin[:, None], pos, f32(0.0))
    ax = [_axis(q[:, a], origin[a], spacing[a], count[a]) for a in range(3)]
    W, S = np.zeros(n, f32), np.zeros((n, 9, 3), f32)
    with np.errstate(all="ignore"):
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    if (dx and count[0] == 1) or (dy and count[1] == 1) or (dz and count[2] == 1):
                        continue
                    p = ((ax[2][0] + dz) * count[1] + (ax[1][0] + dy)) * count[0] + (ax[0][0] + dx)
                    c = sh[p]
                    use = c[:, 0, 3] != 0
                    w = (ax[0][1 + dx] * ax[1][1 + dy]) * ax[2][1 + dz]
                    W = np.where(use, W + w, W)
                    S = np.where(use[:, None, None], S + w[:, None, None] * c[:, :, :3], S)
        E = np.zeros((n, 3), f32)
        for k in range(9):
            y = Y_model(k, nrm[:, 0], nrm[:, 1], nrm[:, 2])
            E = E + (BAND[k] * (S[:, k] / W[:, None])) * y[:, None]
        E = np.where((W != 0)[:, None], E, f32(0.0))
        out = np.fmax(E, f32(0.0))
    out[~fin] = np.nan
    assert out.dtype == f32
    return out


def contract_range_model(sd):
    """in_contract_range of the scene (csrc/rt_types.h, csrc/rt_frame.hip: contract_range) -> a predicate on (n, 3) float32 origins"""
    v = bake.vertex_points(sd)[0].reshape(-1, 3) if sd.n_triangles else np.zeros((0, 3), f32)
    if len(v) == 0:
        return lambda o: np.isfinite(o).all(1)
    lo, hi = v.min(0), v.max(0)
    scale = f32(0.0)
    for a in range(3):
        scale = max(scale, max(hi[a] - lo[a], max(abs(lo[a]), abs(hi[a]))))
    if not scale > 0:
        return lambda o: np.isfinite(o).all(1)
    limit = f32(100.0) * f32(scale)

    def inside(o):
        with np.errstate(all="ignore"):
            out = np.maximum(np.maximum(lo[None, :] - o, o - hi[None, :]), f32(0.0))
            return (out <= limit).all(1)
    return inside


def bake_model(trace, sd, origin, spacing, count, dirs, max_depth, rr_start, seed):
    """The bake as the contract states it: the model's entries, `trace` (OracleScene.trace_paths or Scene.trace_paths) over the entries
    of the probes inside the contract range, the model's projection -> (sh, stats)"""
    e = entries_model(origin, spacing, count, dirs, seed)
    n = len(e["pos"])
    ok = contract_range_model(sd)(e["pos"])
    rad, rays = np.full((n, 3), np.nan, f32), np.full(n, NONE, np.uint32)
    if ok.any():
        out = trace(e["pos"][ok], e["dir"][ok], e["state"][ok], max_depth, samples=1, rr_start=rr_start)
        rad[ok], rays[ok] = out["radiance"], out["rays"]
    return project_model(e["dir"], rad, rays, n // dirs, dirs)


_FALLBACK = []


def fallback_state():
    """The first of the 2^22 consecutive states 1 .. 2^22 whose eight tries are all rejected (about 4.5e-6 of random states are)"""
    if not _FALLBACK:
        for lo in range(1, 1 << 22, 1 << 19):
            s = np.arange(lo, lo + (1 << 19), dtype=np.uint32)
            fb = sphere_dir_model(s)[2]
            if fb.any():
                _FALLBACK.append(int(s[np.flatnonzero(fb)[0]]))
                break
        else:
            _FALLBACK.append(None)
    return _FALLBACK[0]


# ---- the model alone ----------------------------------------------------------------------------------------------------------------------
def test_directions_have_unit_length_and_are_uniform():
    n = 1 << 16
    d, a, fb = sphere_dir_model(entry_states(n, 1, 12345))
    assert (a != 0).all()
    d64 = d.astype(np.float64)
    assert np.abs(np.linalg.norm(d64, axis=1) - 1.0).max() <= 4 * 2.0 ** -23
    # a uniform direction has mean 0 and variance 1/3 per component, and z^2 has mean 1/3 and variance 1/5 - 1/9: five standard errors of n
    assert (np.abs(d64.mean(0)) <= 5 * np.sqrt(1 / 3 / n)).all(), d64.mean(0)
    assert abs((d64[:, 2] ** 2).mean() - 1 / 3) <= 5 * np.sqrt(4 / 45 / n)
    # the draws taken: two per try, so the state is 2 t draws on
    s = entry_states(64, 1, 7)
    after = sphere_dir_model(s)[1]
    ref = s.copy()
    left = np.ones(64, bool)
    for _ in range(2 * TRIES):
        ref = np.where(left, xorshift_model(ref)[1], ref)
        left &= ref != after
    assert not left.any()


def test_a_state_among_2_22_consecutive_ones_exhausts_the_eight_tries():
    s = fallback_state()
    assert s is not None
    d, a, fb = sphere_dir_model(np.array([s], np.uint32))
    assert fb[0]
    ref = np.array([s], np.uint32)
    x = []
    for _ in range(2 * TRIES):  # all sixteen draws stay taken
        u, ref = xorshift_model(ref)
        x.append(f32(-1.0) + f32(2.0) * u[0])
    assert a[0] == ref[0]
    for t in range(TRIES):
        assert not x[2 * t] * x[2 * t] + x[2 * t + 1] * x[2 * t + 1] < 1
    x1, x2 = x[-2] * f32(0.70710677), x[-1] * f32(0.70710677)
    sq = x1 * x1 + x2 * x2
    assert sq <= 1
    np.testing.assert_array_equal(d[0], [(f32(2) * x1) * np.sqrt(f32(1) - sq), (f32(2) * x2) * np.sqrt(f32(1) - sq), f32(1) - f32(2) * sq])
    assert abs(np.linalg.norm(d[0].astype(np.float64)) - 1.0) <= 4 * 2.0 ** -23
    # the seed that makes it entry 0's state (the GPU test's)
    assert entry_states(4, 1, (s - 0x9E3779B9) & 0xFFFFFFFF)[0] == s


def test_entries_model_lays_out_probes_x_fastest_and_entries_probe_major():
    e = entries_model((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), (3, 2, 2), 5, 9)
    assert e["pos"].shape == (60, 3) and e["dir"].shape == (60, 3) and e["state"].shape == (60,)
    np.testing.assert_array_equal(e["pos"][5 * 4], [1.5, 2.25, 3.0])    # probe 4 = (1, 1, 0)
    np.testing.assert_array_equal(e["pos"][5 * 11 + 4], [2.0, 2.25, 5.0])  # probe 11 = (2, 1, 1), its last entry
    assert (e["pos"][:5] == e["pos"][0]).all()
    np.testing.assert_array_equal(e["state"], sphere_dir_model(entry_states(12, 5, 9))[1])


def test_empty_scene_through_the_oracle_gives_the_sky_in_coefficient_zero(oracle):
    sd = scenes.get_scene("empty")
    osc = oracle.OracleScene(sd)
    sky = np.asarray(sd.sky, f32)
    assert (sky > 0).any()
    for dirs in (37, 64):
        sh, stats = bake_model(osc.trace_paths, sd, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 2), dirs, 5, 0, 3)
        assert stats == {"probes": 4, "valid": 4, "rays": 4 * dirs}
        want = (sky * f32(3.5449077)).astype(np.float64)
        got = sh[:, 0, :3].astype(np.float64)
        assert (np.abs(got - want[None, :]) <= dirs * 2.0 ** -23 * np.abs(want)[None, :]).all(), (got, want)
        assert (sh[:, 0, 3] == 1).all() and (sh[:, 1:, 3] == 0).all()
        assert np.abs(sh[:, 1:, :3]).max() < np.abs(want).max()  # the other bands hold sampling noise only


def test_sample_model_returns_a_constant_radiance_for_any_normal():
    g = np.random.default_rng(1)
    count, origin, spacing = (3, 2, 4), (-1.0, 0.5, 2.0), (0.5, 1.5, 0.25)
    L = np.array([0.7, 1.3, 0.02], f32)
    sh = np.zeros((24, 9, 4), f32)
    sh[:, 0, :3] = L * f32(3.5449077)
    sh[:, 0, 3] = 1.0
    n = g.normal(size=(200, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    pos = g.uniform(-3, 4, size=(200, 3)).astype(f32)  # inside and outside
    out = sample_model(origin, spacing, count, sh, pos, n)
    np.testing.assert_allclose(out, np.broadcast_to(L, out.shape), rtol=1e-6)
    sh[5] = 0.0  # an invalid probe drops out of the weights: strictly inside a cell the constant stays
    inner = g.uniform([-0.99, 0.51, 2.01], [-0.01, 1.99, 2.74], size=(200, 3)).astype(f32)
    np.testing.assert_allclose(sample_model(origin, spacing, count, sh, inner, n), np.broadcast_to(L, out.shape), rtol=1e-6)


def test_sample_model_reproduces_a_table_linear_in_x():
    g = np.random.default_rng(2)
    count, origin, spacing = (5, 3, 2), (-1.0, 0.0, 1.0), (0.5, 1.0, 2.0)
    P = probe_positions(origin, spacing, count).astype(np.float64)
    sh = np.zeros((30, 9, 4), f32)
    sh[:, 0, :3] = ((2.0 + 0.75 * P[:, :1]) * [1.0, 2.0, 0.5] / 0.2820948).astype(f32)
    sh[:, 0, 3] = 1.0
    pos = g.uniform([-1, 0, 1], [1, 2, 3], size=(300, 3)).astype(f32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (300, 1))
    want = (2.0 + 0.75 * pos[:, :1].astype(np.float64)) * [1.0, 2.0, 0.5]
    np.testing.assert_allclose(sample_model(origin, spacing, count, sh, pos, nrm), want, rtol=2e-6)
    # outside, the function is that of the clamped point
    far = pos + np.array([10.0, 0.0, 0.0], f32)
    np.testing.assert_allclose(sample_model(origin, spacing, count, sh, far, nrm), np.broadcast_to((2.0 + 0.75) * np.array([1.0, 2.0, 0.5]), want.shape),
                               rtol=2e-6)


def test_sample_model_edges():
    count, origin, spacing = (2, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    sh = np.zeros((2, 9, 4), f32)
    sh[0, 0] = (1.0, 2.0, 3.0, 1.0)
    up = np.array([[0.0, 1.0, 0.0]], f32)
    a = sample_model(origin, spacing, count, sh, np.array([[0.75, 5.0, -5.0]], f32), up)  # only probe 0 is valid: its value, not 1/4 of it
    np.testing.assert_allclose(a[0], np.array([1.0, 2.0, 3.0]) * 0.2820948, rtol=1e-6)
    b = sample_model(origin, spacing, count, sh, np.array([[1.0, 0.0, 0.0]], f32), up)  # on the invalid probe: every weight there, W = 0
    np.testing.assert_array_equal(b, np.zeros((1, 3), f32))
    sh[0, 0, :3] = -1.0
    np.testing.assert_array_equal(sample_model(origin, spacing, count, sh, np.zeros((1, 3), f32), up), np.zeros((1, 3), f32))  # clamped at 0
    bad = sample_model(origin, spacing, count, sh, np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0], [0, 0, 0]], f32),
                       np.array([[0, 1, 0], [0, 1, 0], [0, np.nan, 0], [-np.inf, 0, 0]], f32))
    assert np.isnan(bad).all()


def test_probe_grid_fits_the_bounds():
    sd = scenes.get_scene("cornell")
    origin, count = bake.probe_grid(sd, 0.5, 0.25)
    np.testing.assert_array_equal(origin, np.array([-0.75, -0.75, -0.75], f32))
    assert count == (4, 4, 4)
    assert bake.probe_grid(sd, 0.5)[1] == (5, 5, 5)
    assert bake.probe_grid(sd, 0.5, 1.5)[1] == (1, 1, 1)  # thinner than two margins: one probe at the middle
    np.testing.assert_allclose(bake.probe_grid(sd, 0.5, 1.5)[0], np.zeros(3, f32), atol=1e-6)  # (a wall of the box is a rounding off 1)
    for args in ((0.0,), (0.5, -1.0), (0.001,)):
        with pytest.raises(ValueError):
            bake.probe_grid(sd, *args)
    with pytest.raises(ValueError):
        bake.probe_grid(scenes.get_scene("empty"), 1.0)


# ---- the library in front of the device ------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    """The test that fails without the feature: the thirteen names of the interface (twelve functions and the handle's type)."""
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_probe_volume rt_probe_volume;" in header
    for name in SYMBOLS:
        assert re.search(rf"^(int|void) +{name}\(", header, re.M), name
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    structs = {"rt_probe_volume_desc": (40, ["origin", "spacing", "count", "max_dirs"]),
               "rt_probe_bake_params": (16, ["dirs", "max_depth", "rr_start", "seed"]),
               "rt_probe_stats": (16, ["probes", "valid", "rays"])}
    src = tmp_path / "layout.c"
    body, want = "", []
    for name, (size, fields) in structs.items():
        ct = getattr(abi, name)
        assert [f[0] for f in ct._fields_] == fields and C.sizeof(ct) == size
        body += f'printf("%zu\\n", sizeof({name}));' + "".join(f'printf("%zu\\n", offsetof({name}, {f}));' for f in fields)
        want += [size] + [getattr(ct, f).offset for f in fields]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def _err(lib):
    return lib.rt_last_error().decode()


def _desc(origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), count=(2, 2, 2), max_dirs=64):
    return abi.rt_probe_volume_desc((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*count), max_dirs)


def test_create_refuses_in_the_stated_order_before_any_device_call(rtlib):
    """On a host-only scene no device call can succeed, so every status below was decided in front of the device: RT_ERR_INVALID with the
    cause named, and RT_ERR_NO_DEVICE only for a well-formed request. Each request carries the faults of every later step too, so the word
    in the message shows which check came first."""
    s = Scene(scenes.get_scene("cube"), device=-1)
    h = C.c_void_p(0x1234)
    inv, nan, inf = abi.RT_ERR_INVALID, float("nan"), float("inf")
    steps = [("1 .. 256", {"count": (0, 2, 2)}), ("spacing", {"spacing": (1.0, 0.0, 1.0)}), ("origin", {"origin": (0.0, 0.0, inf)}),
             ("max_dirs", {"max_dirs": 0}), ("2^31", None), ("flag", None)]
    assert rtlib.rt_probe_volume_create(s.h, C.byref(_desc()), 0, None) == inv and "null" in _err(rtlib)
    assert rtlib.rt_probe_volume_create(None, C.byref(_desc(count=(0, 0, 0))), 7, C.byref(h)) == inv and "null scene" in _err(rtlib) and not h.value
    assert rtlib.rt_probe_volume_create(s.h, None, 7, C.byref(h)) == inv and "null description" in _err(rtlib)
    for first in range(4):  # the desc's own faults, each with all the later ones
        kw = {}
        for _, fault in steps[first:4]:
            kw.update(fault)
        h.value = 0x1234
        assert rtlib.rt_probe_volume_create(s.h, C.byref(_desc(**kw)), 7, C.byref(h)) == inv, kw
        assert steps[first][0] in _err(rtlib), (kw, _err(rtlib))
        assert not h.value  # the output is cleared
    for kw, word in (({"count": (257, 1, 1)}, "1 .. 256"), ({"count": (1, 1, 0xFFFFFFFF)}, "1 .. 256"), ({"spacing": (1.0, nan, 1.0)}, "spacing"),
                     ({"spacing": (inf, 1.0, 1.0)}, "spacing"), ({"spacing": (1.0, 1.0, -1.0)}, "spacing"), ({"origin": (nan, 0.0, 0.0)}, "origin"),
                     ({"max_dirs": 65537}, "max_dirs"), ({"count": (256, 256, 256), "max_dirs": 128}, "2^31"),
                     ({"count": (256, 256, 1), "max_dirs": 32768}, "2^31")):
        assert rtlib.rt_probe_volume_create(s.h, C.byref(_desc(**kw)), 0, C.byref(h)) == inv, kw
        assert word in _err(rtlib), (kw, _err(rtlib))
    assert rtlib.rt_probe_volume_create(s.h, C.byref(_desc(count=(256, 256, 256), max_dirs=128)), 7, C.byref(h)) == inv and "2^31" in _err(rtlib)
    assert rtlib.rt_probe_volume_create(s.h, C.byref(_desc()), 1, C.byref(h)) == inv and "flag" in _err(rtlib)
    for kw in ({}, {"count": (1, 1, 1), "max_dirs": 1}, {"count": (256, 256, 256), "max_dirs": 127}, {"count": (3, 2, 2), "max_dirs": 65536},
               {"spacing": (1e-30, 1e30, 1.0), "origin": (-1e30, 1e30, 0.0)}):
        h.value = 0x1234
        assert rtlib.rt_probe_volume_create(s.h, C.byref(_desc(**kw)), 0, C.byref(h)) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in _err(rtlib) and not h.value
    rtlib.rt_probe_volume_destroy(None)
    s.close()


def test_calls_refuse_null_handles_before_any_device_call(rtlib):
    inv = abi.RT_ERR_INVALID
    buf = np.zeros(64, f32)
    words = np.zeros(16, np.uint32)
    p = abi.rt_probe_bake_params(4, 5, 0, 1)
    st = abi.rt_probe_stats()
    calls = [lambda: rtlib.rt_probe_volume_entries(None, C.byref(p), abi.fptr(buf), abi.fptr(buf), abi.u32ptr(words)),
             lambda: rtlib.rt_probe_volume_entries_device(None, C.byref(p), None, None, None, None),
             lambda: rtlib.rt_probe_volume_bake(None, C.byref(p), abi.fptr(buf), C.byref(st)),
             lambda: rtlib.rt_probe_volume_bake(None, None, None, None),
             lambda: rtlib.rt_probe_volume_bake_device(None, C.byref(p), None, None, None),
             lambda: rtlib.rt_probe_volume_set_sh(None, abi.fptr(buf)),
             lambda: rtlib.rt_probe_volume_set_sh_device(None, None, None),
             lambda: rtlib.rt_probe_volume_get_sh(None, abi.fptr(buf)),
             lambda: rtlib.rt_probe_volume_get_sh_device(None, None, None),
             lambda: rtlib.rt_probe_volume_sample(None, 4, abi.fptr(buf), abi.fptr(buf), abi.fptr(buf)),
             lambda: rtlib.rt_probe_volume_sample(None, 0, None, None, None),
             lambda: rtlib.rt_probe_volume_sample_device(None, 4, None, None, None, None)]
    for k, call in enumerate(calls):
        assert call() == inv, k
        assert "null" in _err(rtlib), (k, _err(rtlib))


def test_python_wrapper_refuses_wrong_shapes(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    for good in (((0, 0, 0), 1.0, (2, 2, 2)), (np.zeros(3, f32), (1.0, 2.0, 3.0), np.array([1, 1, 1])), ([0.5, 0, 0], np.float32(0.25), [3, 2, 2])):
        with pytest.raises(abi.RtError) as e:
            ProbeVolume(s, *good)
        assert e.value.status == abi.RT_ERR_NO_DEVICE
    for bad in (((0, 0), 1.0, (2, 2, 2)), ((0, 0, 0), (1.0, 2.0), (2, 2, 2)), ((0, 0, 0), 1.0, (2, 2)), ((0, 0, 0), 1.0, (2.0, 2.0, 2.0)),
                ((0, 0, 0), 1.0, (2, -1, 2)), ((0, 0, 0), 1.0, (2, 2, 1 << 32))):
        with pytest.raises(ValueError):
            ProbeVolume(s, *bad)
    with pytest.raises(ValueError):
        ProbeVolume(s, (0, 0, 0), 1.0, (2, 2, 2), max_dirs=-1)
    for kw, args in (({}, ((0, 0, 0), 0.0, (2, 2, 2))), ({}, ((0, 0, 0), 1.0, (0, 2, 2))), ({"max_dirs": 0}, ((0, 0, 0), 1.0, (2, 2, 2))),
                     ({"max_dirs": 65537}, ((0, 0, 0), 1.0, (2, 2, 2))), ({}, ((0, float("nan"), 0), 1.0, (2, 2, 2)))):
        with pytest.raises(abi.RtError) as e:
            ProbeVolume(s, *args, **kw)
        assert e.value.status == abi.RT_ERR_INVALID
    import rtamd
    assert rtamd.ProbeVolume is ProbeVolume
    s.close()
