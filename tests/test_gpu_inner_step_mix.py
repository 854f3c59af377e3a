"""The mixed-precision plane decode of the one-launch kernels (csrc/rt_device.h: trav_inner<.., .., true>, trav_begin<true>) on the
GPU. The step makes the 24 plane bytes of a node halves (v_perm_b32) and feeds them to v_fma_mix_f32 on scale / d * 2^24: every plane distance
is the other kernels' fma((float)q, a, b) bit for bit, so no node visit, triangle test, hit, frame or ray count may change. Both one-launch
renderers are held to the CPU oracle, bit for bit on the fp32 frame, the unorm8 image and the ray count:
  - the atrium at detail 1 and the Cornell box;
  - the stack of 1,024 sheets of tests/test_gpu_inner_step_masks.py, where a lane's stack runs past its LDS entries (the general push / pop path);
  - a room 1e5 across. Its nodes' grid steps are 2^9: under the clamp of the other kernels (|d| >= 1e-30) scale / d * 2^24 overflows for a
    direction component that is zero, 0 * inf is NaN and the child with q = 0 is lost; the kernels with this step clamp to 2^-83. A camera cannot
    send a ray exactly along an axis (every camera ray is jittered), but with a focal length of 1e-9 the z component of EVERY camera ray is
    zero as a half: all of them run in the plane z = const, through the room's whole width.
A batch of rays with one direction component at 0, +-1e-32, +-1e-27 and +-1e-24 (all zero as halves, as every ray's direction is stored) from
100 scene scales beyond the scene (the farthest origin the contract allows) goes through rt_intersect_batch and the closest-hit query, whose kernel keeps the converting step and the 1e-30 clamp, against brute force.
With RT_KERNEL_STATS=1 the instrumented instantiations report node visits and triangle tests per ray: on the small atrium frame they are the
numbers of the commit before this step, digit for digit."""
import re

import numpy as np
import pytest

from rtamd import abi
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer
from rtamd.scenes import CameraPose, Material, SceneBuilder, mesh_quad
from test_gpu_inner_step_masks import K_LDS_STACK, KINDS, _hold, first_descent_stack, host_tree, sheets_scene, tubes_scene
from test_gpu_ray_query import NO_TRI, assert_closest

pytestmark = pytest.mark.gpu
f32 = np.float32
# node visits (inner steps) and triangle tests per ray of the 64 x 36 atrium frame below, as the commit before the mixed step reports them
PARENT_STATS = {"WavefrontRenderer": (34038, "13.12", "1.68"), "MegakernelRenderer": (34154, "13.14", "1.67")}  # rays, visits, tests


def big_room_scene(focal):
    """a closed room [0, 1e5]^3 with a lamp under its ceiling, a metal partition and a red block; the camera in its middle looks along -z"""
    sb = SceneBuilder("big_room")
    white = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.73, 0.73, 0.73)))
    red = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.65, 0.05, 0.05)))
    metal = sb.add_material(Material(abi.RT_MAT_METALLIC, (0.9, 0.85, 0.7), roughness=0.1))
    lamp = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.78, 0.78, 0.78), emissive=(6.0, 6.0, 6.0)))
    L = 1.0e5
    q = lambda m, *a: sb.add_instance(sb.add_mesh(*mesh_quad(*a, nx=4, ny=4)), m)
    q(white, (0, 0, L), (L, 0, L), (L, 0, 0), (0, 0, 0))      # floor
    q(white, (0, L, 0), (L, L, 0), (L, L, L), (0, L, L))      # ceiling
    q(white, (0, 0, 0), (L, 0, 0), (L, L, 0), (0, L, 0))      # back
    q(white, (L, 0, L), (0, 0, L), (0, L, L), (L, L, L))      # front
    q(red, (0, 0, L), (0, 0, 0), (0, L, 0), (0, L, L))        # left
    q(metal, (L, 0, 0), (L, 0, L), (L, L, L), (L, L, 0))      # right
    q(lamp, (2.5e4, 9.9e4, 2.5e4), (7.5e4, 9.9e4, 2.5e4), (7.5e4, 9.9e4, 7.5e4), (2.5e4, 9.9e4, 7.5e4))
    q(metal, (3e4, 0, 3e4), (6e4, 0, 3e4), (6e4, 5e4, 3e4), (3e4, 5e4, 3e4))
    q(red, (1e4, 0, 6e4), (2e4, 0, 6e4), (2e4, 3e4, 6e4), (1e4, 3e4, 6e4))
    sb.camera = CameraPose((5.0e4, 4.0e4, 9.0e4), (0.0, 0.0, -1.0), focal)
    return sb.build()


def test_the_atrium(rtlib, oracle, scene_cache):
    sd = scene_cache("atrium", detail=1)
    scene = Scene(sd, device=0)
    try:
        _hold(scene, sd, oracle.OracleScene(sd), oracle, 64, 36, 4, 4, use_bvh=True)
    finally:
        scene.close()


def test_the_cornell_box(rtlib, oracle, scene_cache):
    sd = scene_cache("cornell")
    scene = Scene(sd, device=0)
    try:
        _hold(scene, sd, oracle.OracleScene(sd), oracle, 64, 64, 4, 5)
    finally:
        scene.close()


def test_a_stack_past_its_lds_entries(rtlib, devlib, oracle):
    sd = sheets_scene()
    deep = first_descent_stack(host_tree(devlib, sd)["nodes"], float(sd.camera.position[2]))
    assert deep > K_LDS_STACK, f"{deep} entries on the stack of a ray along the sheets' axis: not past the {K_LDS_STACK} in LDS"
    scene = Scene(sd, device=0)
    try:
        _hold(scene, sd, oracle.OracleScene(sd), oracle, 16, 16, 4, 5)
    finally:
        scene.close()


@pytest.mark.parametrize("focal", [1.0, 1e-9])
def test_a_room_1e5_across(rtlib, devlib, oracle, focal):
    sd = big_room_scene(focal)
    nodes = host_tree(devlib, sd)["nodes"]
    steps = np.abs(nodes[:, [3, 10, 11]].view(f32))
    assert steps.max() >= 256.0, "grid steps of 2^8 and more: scale * 1e30 * 2^24 is not finite"
    if focal < 1.0:  # every camera ray's z component is zero as a half
        cam = Camera.for_scene(sd, (8, 8))
        assert np.float16(f32(cam.c.pixel00[2]) - f32(cam.c.center[2])) == 0 and cam.c.delta_u[2] == 0 and cam.c.delta_v[2] == 0
    scene = Scene(sd, device=0)
    try:
        _hold(scene, sd, oracle.OracleScene(sd), oracle, 24, 16, 4, 4)
    finally:
        scene.close()


def test_rays_with_a_vanishing_direction_component_from_100_diameters(rtlib, oracle):
    sd = tubes_scene()
    tw = sd.world_triangles().reshape(-1, 3)
    lo, hi = tw.min(0), tw.max(0)
    lo, hi = lo.astype(f32), hi.astype(f32)
    scale = f32(max(max(hi[a] - lo[a], abs(lo[a]), abs(hi[a])) for a in range(3)))  # the contract's scene scale (include/rt_mi355x.h: rt_intersect_batch)
    limit = f32(100.0) * scale

    def far(a, side):  # the farthest origin the contract allows beyond the scene on axis a
        edge = hi[a] if side > 0 else lo[a]
        o = f32(edge + f32(side) * limit)
        while f32(abs(f32(o - edge))) > limit:
            o = np.nextafter(o, edge)
        return o

    tiny = [0.0] + [s * v for v in (1e-32, 1e-27, 1e-24) for s in (1.0, -1.0)]
    org, dirs = [], []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (1.0, -1.0):
            for a in np.linspace(lo[u] - 0.25, hi[u] + 0.25, 9):
                for b in np.linspace(lo[v] - 0.25, hi[v] + 0.25, 9):
                    for k, c in enumerate(tiny):
                        o = np.zeros(3)
                        o[axis] = far(axis, side)
                        o[u], o[v] = a, b
                        d = np.zeros(3)
                        d[axis] = -side
                        d[u if k % 2 else v] = c  # the vanishing component, on either of the other axes
                        org.append(o), dirs.append(d)
    org, dirs = np.array(org, f32), np.array(dirs, f32)
    assert np.all((dirs.astype(np.float16) == 0).sum(1) == 2), "every tiny component is zero as a half"
    osc = oracle.OracleScene(sd)
    e = osc.intersect(org, dirs, use_bvh=False)
    hit = e[3] != NO_TRI
    assert 0.2 < hit.mean() < 0.9
    scene = Scene(sd, device=0)
    try:
        assert_closest(scene.intersect(org, dirs), e, "rt_intersect_batch")
        assert_closest(scene.trace(org, dirs), e, "closest-hit query")
    finally:
        scene.close()


def test_node_visits_and_triangle_tests_are_the_parents(rtlib, scene_cache, monkeypatch, capfd):
    monkeypatch.setenv("RT_KERNEL_STATS", "1")
    sd = scene_cache("atrium", detail=1)
    cam = Camera.for_scene(sd, (64, 36))
    scene = Scene(sd, device=0)
    seen = {}
    try:
        for cls, _ in KINDS:
            r = cls(scene, (64, 36), 4, 4)
            try:
                fr = r.render_frame(cam)
            finally:
                r.close()
            m = re.findall(r"per ray: ([0-9.]+) inner \(.*?\), ([0-9.]+) tri", capfd.readouterr().err)
            assert m, "no [rt stats] report"
            seen[cls.__name__] = (fr.rays, m[-1][0], m[-1][1])
    finally:
        scene.close()
    with capfd.disabled():
        print("atrium 64 x 36, 4 spp, depth 4: rays, node visits, triangle tests per ray:", seen)
    assert seen == PARENT_STATS
