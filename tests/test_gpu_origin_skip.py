"""The origin skip on the GPU (csrc/rt_types.h: SkipRec; rt_device.h: trav_inner<true>): k_megakernel and k_wf_finish do not
descend into the flat subtree a bounce ray starts on. The cull must be exact, so every case renders a small frame with both renderers and
holds the fp32 frame, the unorm8 image and the ray count against the brute-force CPU oracle, bit for bit: scenes where the skip takes
much (two-triangle walls), where it must let a ray through to a surface a hair away (gaps around kTNear), where |n . d| straddles the
threshold (a grazing camera), where rays start on a face and go INWARD (glass), where nothing is coplanar (a column), with forced pixel
slices, and on the scenes whose table holds only the no-match word (updatable, before and after an update; built on the device)."""
import ctypes as C
import re

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer
from rtamd.scenes import CameraPose, Material, SceneBuilder, mesh_box, mesh_cylinder, mesh_quad, trs

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = 64, 48, 8, 6
SKIP_NONE = 1


def _room(sb, light=True):
    """a box room of two-triangle walls (each wall's leaf is the whole wall), open to the camera at +z"""
    white = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.73, 0.73, 0.73)))
    red = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.65, 0.05, 0.05)))
    metal = sb.add_material(Material(abi.RT_MAT_METALLIC, (0.9, 0.85, 0.7), roughness=0.1))
    q = lambda *a, **k: sb.add_mesh(*mesh_quad(*a, **k))
    sb.add_instance(q((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1)), white)
    sb.add_instance(q((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), white)
    sb.add_instance(q((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), metal)
    sb.add_instance(q((-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1)), red)
    sb.add_instance(q((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), white)
    if light:
        lamp = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.78, 0.78, 0.78), emissive=(15.0, 15.0, 15.0)))
        sb.add_instance(q((-0.25, 0.995, -0.25), (0.25, 0.995, -0.25), (0.25, 0.995, 0.25), (-0.25, 0.995, 0.25)), lamp)
    sb.camera = CameraPose((0.0, 0.0, 3.4), (0.0, 0.0, -1.0), 2.0)
    return white


def room_scene():
    sb = SceneBuilder("room")
    _room(sb)
    return sb.build()


def planes_scene(gap):
    """a floor tessellated 6 x 6 and a second sheet `gap` above its middle: a ray that leaves the floor must still find the sheet"""
    sb = SceneBuilder(f"planes_{gap}")
    white = _room(sb)
    blue = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.1, 0.2, 0.8)))
    sb.add_instance(sb.add_mesh(*mesh_quad((-0.9, -0.9, 0.9), (0.9, -0.9, 0.9), (0.9, -0.9, -0.9), (-0.9, -0.9, -0.9), nx=6, ny=6)), white)
    y = -0.9 + gap
    sb.add_instance(sb.add_mesh(*mesh_quad((-0.5, y, 0.5), (0.5, y, 0.5), (0.5, y, -0.5), (-0.5, y, -0.5), nx=3, ny=3)), blue)
    sb.camera = CameraPose((0.0, 0.6, 3.0), (0.0, -0.45, -1.0), 2.0)
    return sb.build()


def grazing_scene():
    """the camera looks along a tessellated floor at under 1 degree: mirror-like bounces leave it with |n . d| around the entries' thresholds"""
    sb = SceneBuilder("grazing")
    gloss = sb.add_material(Material(abi.RT_MAT_METALLIC, (0.9, 0.9, 0.9), roughness=0.02))
    white = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.7, 0.7, 0.7)))
    sb.add_instance(sb.add_mesh(*mesh_quad((-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), nx=8, ny=8)), gloss)
    sb.add_instance(sb.add_mesh(*mesh_quad((-4, 0, -4), (4, 0, -4), (4, 3, -4), (-4, 3, -4), nx=2, ny=2)), white)
    sb.camera = CameraPose((0.0, 0.03, 3.9), (0.0, -0.008, -1.0), 1.2)  # atan(0.008) = 0.46 degrees
    return sb.build()


def slab_scene():
    sb = SceneBuilder("slab")
    _room(sb)
    glass = sb.add_material(Material(abi.RT_MAT_DIELECTRIC, ior=1.5))
    sb.add_instance(sb.add_mesh(*mesh_box()), glass, trs((0.0, -0.2, 0.0), s=(0.6, 0.5, 0.08)))
    return sb.build()


def column_scene():
    sb = SceneBuilder("column")
    white = _room(sb)
    sb.add_instance(sb.add_mesh(*mesh_cylinder(24, 6, radius=0.35, height=1.9)), white, trs((0.0, -0.98, 0.0)))
    return sb.build()


CASES = {
    "room": room_scene,
    "planes_5e-5": lambda: planes_scene(5e-5),
    "planes_2e-4": lambda: planes_scene(2e-4),
    "planes_1e-3": lambda: planes_scene(1e-3),
    "grazing": grazing_scene,
    "slab": slab_scene,
    "column": column_scene,
}


def _oracle_frames(oracle, sd):
    osc = oracle.OracleScene(sd)
    ocam = oracle.camera(W, H, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    return {kind: osc.render(ocam, kind, DEPTH, SPP, use_bvh=False) for kind in (abi.RT_RENDERER_WAVEFRONT, abi.RT_RENDERER_MEGAKERNEL)}


def _hold(scene, sd, want, slices=-1):
    cam = Camera.for_scene(sd, (W, H))
    for cls, kind in ((WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT), (MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL)):
        r = cls(scene, (W, H), DEPTH, SPP)
        if slices >= 0:
            r.set_schedule(pixel_slices=slices)
        fr = r.render_frame(cam)
        f, b, rays = want[kind]
        bad = int((fr.rgba_f32 != f).any(-1).sum())
        r.close()
        assert fr.rays == rays, f"{cls.__name__}: {fr.rays} rays, the oracle {rays}"
        assert bad == 0, f"{cls.__name__}: {bad} pixels differ from the oracle"
        assert np.array_equal(fr.rgba_f32, f) and np.array_equal(fr.rgba_u8, b)
        if slices >= 2:
            assert fr.pixel_slices == slices
    return True


def _skip_words(devlib, sd, kind=abi.RT_BVH_DEFAULT, device=-1):
    c = sd.to_c()
    h = C.c_void_p()
    abi.check(devlib.rt_scene_create(C.byref(c), device, kind, C.byref(h)), devlib)
    n = C.c_uint32(0)
    words = np.zeros((sd.n_triangles, 8), np.uint32)
    abi.check(devlib.rt_dev_scene_skip_table(h, C.byref(n), abi.u32ptr(words), sd.n_triangles, 0), devlib)
    abi.check(devlib.rt_scene_check_bvh(h), devlib)
    devlib.rt_scene_destroy(h)
    return words[:, 0]


@pytest.fixture(scope="module")
def room(oracle):
    sd = room_scene()
    return sd, _oracle_frames(oracle, sd)


@pytest.mark.parametrize("name", list(CASES))
def test_frames_with_the_skip_are_the_oracles_bit_for_bit(rtlib, devlib, oracle, name):
    sd = CASES[name]()
    words = _skip_words(devlib, sd)
    if name != "column":  # (the column: facets of 12 coplanar triangles, 15 degrees between neighbours — the proof must stop at a facet: _skip_words runs the checker)
        assert np.mean(words != SKIP_NONE) > 0.5, "the flat walls must be in the table, or the case tests nothing"
    scene = Scene(sd, device=0)
    try:
        _hold(scene, sd, _oracle_frames(oracle, sd))
    finally:
        scene.close()


def test_a_frame_in_forced_slices(rtlib, room):
    sd, want = room
    scene = Scene(sd, device=0)
    try:
        _hold(scene, sd, want, slices=4)
    finally:
        scene.close()


def test_an_updatable_scene_before_and_after_an_update(rtlib, oracle, room):
    sd, want = room
    scene = Scene(sd, device=0, updatable=True)
    try:
        _hold(scene, sd, want)
        xf = sd.transforms.copy().reshape(-1, 16)
        xf[2] = trs((0.0, 0.0, -0.2), scenes.quat_axis_angle((0, 1, 0), 0.2)).reshape(16)  # the back wall moves and turns: no longer where a table would say
        nm = np.stack([scenes.normal_matrix(m) for m in xf]).reshape(-1, 9)
        scene.update(instances=(xf, nm))
        scene.check_bvh()
        _hold(scene, scene.desc, _oracle_frames(oracle, scene.desc))
    finally:
        scene.close()


def test_a_device_built_tree_skips_nothing_and_renders_the_same(rtlib, devlib, oracle):
    sd = planes_scene(2e-4)
    assert np.all(_skip_words(devlib, sd, abi.RT_BVH_LBVH_GPU, device=0) == SKIP_NONE)
    scene = Scene(sd, device=0, bvh=abi.RT_BVH_LBVH_GPU)
    try:
        _hold(scene, sd, _oracle_frames(oracle, sd))
    finally:
        scene.close()


def test_the_device_takes_the_skip(rtlib, monkeypatch, capfd):
    """A frame that matches the oracle says nothing about whether the skip is taken. The instrumented instantiations (RT_KERNEL_STATS=1)
    count node visits and triangle tests per ray: the same scene built static (with its table) and updatable (no-match words only) traces
    the same rays, and the static one must visit fewer nodes and test fewer triangles."""
    sd = planes_scene(1e-3)
    cam = Camera.for_scene(sd, (W, H))
    monkeypatch.setenv("RT_KERNEL_STATS", "1")
    for cls in (MegakernelRenderer, WavefrontRenderer):
        seen = {}
        for updatable in (False, True):
            scene = Scene(sd, device=0, updatable=updatable)
            try:
                r = cls(scene, (W, H), DEPTH, SPP)
                fr = r.render_frame(cam)
                r.close()
            finally:
                scene.close()
            m = re.findall(r"per ray: ([0-9.]+) inner \(.*?\), ([0-9.]+) tri", capfd.readouterr().err)
            assert m, "no [rt stats] report"
            seen[updatable] = (fr.rays, float(m[-1][0]), float(m[-1][1]))
        print(cls.__name__, "rays, node visits, triangle tests per ray: with the table", seen[False], "without", seen[True])
        assert seen[False][0] == seen[True][0]
        assert seen[False][1] < seen[True][1] and seen[False][2] < seen[True][2]
