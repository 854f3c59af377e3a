"""k_closest (rt_closest.hip) on the trees and records its own inner and leaf steps have to get right — its decode of the child planes and
its lb, the test of the child word against kChildEmpty, the sorting network on (lb, child), the LDS stack with the wave-uniform switch to
the spill routines, the two-record leaf with the winner rule: deep stacks, NaN candidates and slivers in deep leaves, pre-split triangles,
duplicate triangles, the median fallback, a tree that lies whole in the LDS top, scenes away from the origin, the corner of the contract
range, more entries than the persistent grid has lanes, radii on an answer of zero. Every comparison is bit for bit (same); the expected
values are rt_scene_closest_host(use_bvh = 0) on the same scene object and, where stated, closest_model — never the kernel's own output.
The scenes are tests/closest_scenes.py's; tests/test_closest_points.py states the same facts for the host walk."""
import numpy as np
import pytest

import closest_scenes as cs
from rtamd import abi, scenes
from rtamd.renderer import Scene
from test_closest_points import NO_TRI, OUTPUTS, closest_model, point_mix, same, world_vertices
from test_gpu_closest_points import closest_dev, host_form

pytestmark = pytest.mark.gpu
f32 = np.float32
_models = {}


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    return 0


def model_of(key, pos, wv):
    """closest_model without a radius, computed once per point set and shared by the builders (it takes seconds on the mixed scene)"""
    if key not in _models:
        _models[key] = closest_model(pos, wv)
    return _models[key]


def hold(s, pos, what, seed=5, model=None, wv=None):
    """The device form and the host form equal the host brute force on the same scene, with no radius and with radius_mix around the
    unbounded answer; with `model` (closest_model without a radius) the brute force equals it, and with radii the model on the first 1,024
    entries. -> the brute force's results, without and with radii"""
    want = s.closest_host(pos)
    same(closest_dev(s, pos), want, f"{what}: device")
    same(host_form(s, pos), want, f"{what}: host form")
    md2 = cs.radius_mix(want["dist2"], seed)
    want_r = s.closest_host(pos, md2)
    same(closest_dev(s, pos, md2), want_r, f"{what}: device, radius_mix")
    same(host_form(s, pos, md2), want_r, f"{what}: host form, radius_mix")
    hit = want_r["tri"] != NO_TRI
    assert (want["tri"] != NO_TRI).all() and hit.any() and (~hit).any()
    if model is not None:
        same(want, model, f"{what}: brute force vs model")
        same({k: want_r[k][:1024] for k in OUTPUTS}, closest_model(pos[:1024], wv, md2[:1024]), f"{what}: brute force vs model, radius_mix")
    return want, want_r


# ---- deep stacks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh", "lbvh_gpu"])
def test_the_pile_spills_the_point_stack_and_equals_the_brute_force(gpu, devlib, monkeypatch, builder):
    """The pile of test_gpu_parity.py's deep-stack test: a point with no radius enters every child on its first descent and pushes three
    words per level, so the tree's stack_need — asserted > kLdsStack on the very tree the kernel walks — is reached and the lanes go
    through the spill routines. 4,096 points of the mix and 1,024 in the free corner above and below the pile. Then one wave (n = 64 under
    RT_CLOSEST_GRID=1) whose even entries have max_dist2 = -1 — the root is visited, nothing is entered, the sentinel is popped — while the
    odd ones have no radius: shallow and spilled lanes in the same step."""
    sd = cs.pile_scene()
    s = Scene(sd, gpu, cs.BUILDERS[builder], lib=devlib)
    tree = s.tree()
    assert tree["stack_need"] > cs.K_LDS_STACK and tree["built_by"] == cs.BUILDERS[builder]
    s.check_bvh()
    pos = np.concatenate([point_mix(sd, 4096, 1), cs.pile_corner_points(1024, 2)])
    want, _ = hold(s, pos, f"pile {builder}")
    assert len(np.unique(want["tri"])) > 100
    s.close()
    monkeypatch.setenv("RT_CLOSEST_GRID", "1")  # (read at a scene's first launch)
    s = Scene(sd, gpu, cs.BUILDERS[builder], lib=devlib)
    assert s.tree()["stack_need"] > cs.K_LDS_STACK
    few = np.ascontiguousarray(cs.pile_corner_points(1024, 2)[::16])
    md2 = np.where(np.arange(64) % 2 == 0, f32(-1.0), f32(np.inf)).astype(f32)
    want = s.closest_host(few, md2)
    assert ((want["tri"] == NO_TRI) == (np.arange(64) % 2 == 0)).all()
    same(closest_dev(s, few, md2), want, f"pile {builder}: one wave, shallow and spilled lanes")
    s.close()


# ---- NaN candidates and slivers in deep leaves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh", "lbvh_gpu"])
@pytest.mark.parametrize("points", ["mix", "corner"])
def test_the_mixed_scene_with_degenerate_triangles_equals_the_brute_force_and_the_model(gpu, points, builder):
    """Two scene-spanning triangles over 3,000 tiny ones, 500 slivers and 300 degenerate triangles, a hundred of which give NaN candidates
    (tests/test_closest_points.py asserts that on the model): leaves of two records deep in the tree whose dist2 is NaN, pre-split triangles
    under SAH whose index sits in several leaves. At the point mix and in the corner of the contract range, 99.9 scales out on all three
    axes, where the host form accepts every point (it refuses a call with one point outside)."""
    sd, mask = cs.mixed_scene()
    wv = world_vertices(sd)
    s = Scene(sd, gpu, cs.BUILDERS[builder])
    assert (s.info().n_split_triangles > 0) == (builder == "sah")
    s.check_bvh()
    pos = point_mix(sd, 4096, 7) if points == "mix" else cs.corner_points(sd, 4096, 3)
    want, _ = hold(s, pos, f"mixed {builder} {points}", model=model_of(points, pos, wv), wv=wv)
    assert not np.isnan(want["dist2"]).any()
    if points == "mix":
        assert mask[want["tri"]].sum() >= 1
    s.close()


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_duplicate_triangles_tie_and_the_lowest_copy_wins(gpu, builder):
    """Seven shuffled copies of the cube: every candidate ties with six others bit for bit, in the winner rule and as equal keys in the
    sorting network. Against the model and against the lowest-copy rule, computed from the permutation alone."""
    sd = cs.duplicate_scene()
    wv = world_vertices(sd)
    s = Scene(sd, gpu, cs.BUILDERS[builder])
    pos = point_mix(sd, 4096, 4)
    want, want_r = hold(s, pos, f"duplicates {builder}", model=model_of("duplicates", pos, wv), wv=wv)
    got, hit = closest_dev(s, pos), want_r["tri"] != NO_TRI
    np.testing.assert_array_equal(got["tri"], cs.lowest_copy(got["tri"]))
    np.testing.assert_array_equal(want_r["tri"][hit], cs.lowest_copy(want_r["tri"][hit]))
    assert len(np.unique(got["tri"])) == 12
    s.close()


def test_the_median_fallback_with_forty_equal_triangles(gpu, devlib):
    """chain_scene (tests/test_scene_update.py): the host LBVH falls back to the balanced tree, and 41 equal triangles tie."""
    from test_scene_update import chain_scene
    sd = chain_scene()
    wv = world_vertices(sd)
    s = Scene(sd, gpu, abi.RT_BVH_LBVH, lib=devlib)
    assert s.tree()["built_by"] == abi.RT_BVH_MEDIAN_INTERNAL
    pos = point_mix(sd, 4096, 6)
    hold(s, pos, "chain", model=model_of("chain", pos, wv), wv=wv)
    s.close()


# ---- every node from the LDS top, and every builder the host walk is held on ----------------------------------------------------------------
def _updated(gpu):
    from test_scene_update import update_sequence
    sd = scenes.get_scene("atrium", detail=1)
    s = Scene(sd, gpu, abi.RT_BVH_LBVH, updatable=True)
    for u in update_sequence(sd)[:2]:
        s.update(**u)
    return s


TREES = {
    "tables": lambda gpu: Scene(scenes.table_scene(), gpu, abi.RT_BVH_SAH),
    "sah_presplit": lambda gpu: Scene(scenes.atrium_tilted_scene(1), gpu, abi.RT_BVH_SAH),
    "atrium_host_lbvh": lambda gpu: Scene(scenes.get_scene("atrium", detail=1), gpu, abi.RT_BVH_LBVH),
    "updated_lbvh": _updated,
}


@pytest.mark.parametrize("case", list(TREES))
def test_the_builders_the_host_walk_is_held_on(gpu, case):
    """The table scene, whose whole tree is staged in LDS (n_nodes <= kTopNodes: no node is fetched from memory); the tilted atrium under
    SAH with pre-split triangles; the atrium under the host LBVH; an updatable LBVH atrium after two updates (refitted boxes)."""
    s = TREES[case](gpu)
    info = s.info()
    if case == "tables":
        assert 1 < info.n_nodes <= cs.K_TOP_NODES
    if case == "sah_presplit":
        assert info.n_split_triangles > 0
    s.check_bvh()
    hold(s, point_mix(s.desc, 4096, 8), case)
    s.close()


# ---- away from the origin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh_gpu"])
@pytest.mark.parametrize("off", cs.OFFSETS, ids=["near", "far"])
def test_the_atrium_away_from_the_origin(gpu, off, builder):
    """The atrium moved to (1000, -2000, 500) and to (1e5, 1e5, 1e5): the scene scale, and with it the contract range, the padding and the
    node grids, is the offset's, 30 and 3,000 times the extent."""
    sd = cs.offset_scene(off)
    s = Scene(sd, gpu, cs.BUILDERS[builder])
    s.check_bvh()
    hold(s, point_mix(sd, 4096, 2), f"offset {off} {builder}")
    s.close()


# ---- more entries than the grid has lanes, product library ----------------------------------------------------------------------------------
def test_every_wave_of_the_product_grid_claims_again(gpu, scene_cache):
    """n = 2^20 + 17 on the Cornell box in the product library, whose persistent grid is at most three 512-thread workgroups per CU: n is
    asserted above that many lanes, so every wave refills beside live lanes, and the last chunk is a partial one. All five outputs."""
    import torch
    n = (1 << 20) + 17
    assert n > 3 * 512 * torch.cuda.get_device_properties(0).multi_processor_count
    sd = scene_cache("cornell")
    s = Scene(sd, gpu)
    pos = point_mix(sd, n, 9)
    want = s.closest_host(pos)
    same(closest_dev(s, pos), want, "2^20 + 17 entries: device")
    same(host_form(s, pos), want, "2^20 + 17 entries: host form")
    assert (want["tri"] != NO_TRI).all() and len(np.unique(want["tri"])) == sd.n_triangles
    s.close()


# ---- radii on the answer's zero -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_radii_of_signed_zero_and_the_smallest_normal_on_vertices(gpu, scene_cache, name):
    """The scene's first 1,000 vertices (the Cornell box: all of them) as points with max_dist2 cycling through -0.0, +0.0, FLT_MIN, +inf
    and -1: the first four hit with dist2 == 0 and the vertex as point, -1 misses — as the model says, whose statement check_vertex_radii
    verifies (on the mixed scene for v0 and v1 of a triangle: it says why a third vertex need not be at 0)."""
    sd = scene_cache("cornell") if name == "cornell" else cs.mixed_scene()[0]
    wv = world_vertices(sd)
    pos, md2 = cs.vertex_radii(wv, min(1000, 3 * len(wv) // 5 * 5))
    want = closest_model(pos, wv, md2)
    cs.check_vertex_radii(want, pos, md2, name, third_vertices=name == "cornell")
    for builder in ("sah", "lbvh_gpu"):
        s = Scene(sd, gpu, cs.BUILDERS[builder])
        same(s.closest_host(pos, md2), want, f"{name} {builder}: brute force vs model")
        same(closest_dev(s, pos, md2), want, f"{name} {builder}: device")
        same(host_form(s, pos, md2), want, f"{name} {builder}: host form")
        s.close()
