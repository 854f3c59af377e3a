"""The device refit (csrc/rt_update.hip) held to the host refit, its CPU reference, where the device path has the most room to drift: the
full-size atrium (1,106 reduction workgroups), bounds attained at 0 by both signed zeros, every kind of update, round trips, non-finite
refusals, shading tables across their LDS and packed-word limits, and the host builders' deep trees. Bit for bit unless stated."""
import math

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer
from test_gpu_parity import TABLE_CASES
from test_scene_update import (ZERO_CASES, _exact_union_builders, _status, _tables_equal, _tree_equal, chain_scene, get_scene,
                               last_leaf_count, model_node_words, rays, same_bits, signed_zero_scene, signed_zero_starts, spin_about_centre, update_sequence,
                               zero_case_id)

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, DEPTH, SPP = 48, 32, 5, 4
RENDERERS = (MegakernelRenderer, WavefrontRenderer)


def frame(cls, scene, cam, size=(W, H), depth=DEPTH, spp=SPP):
    r = cls(scene, size, depth, spp)
    fr = r.render_frame(cam)
    r.close()
    return fr


def assert_same_frame(a, b, what=""):
    assert a.rays == b.rays, what
    np.testing.assert_array_equal(a.rgba_f32, b.rgba_f32, err_msg=what)
    np.testing.assert_array_equal(a.rgba_u8, b.rgba_u8, err_msg=what)


def assert_same_hits(a, b, org, d):
    for x, y in zip(a.intersect(org, d), b.intersect(org, d)):
        assert same_bits(x, y)


def assert_model_words(lib, tree):
    words, live = model_node_words(lib, tree)
    assert same_bits(tree["nodes"][live, :12], words[live])


def assert_fresh_bounds(s, bvh, lib):
    ftree = Scene(s.desc, -1, bvh, lib=lib).tree()
    tree = s.tree()
    for k in ("wverts", "pad", "bounds_lo", "bounds_hi"):
        assert same_bits(tree[k], ftree[k]), k


# ---- 1. the full-size atrium --------------------------------------------------------------------------------------------------------------
STRIP = dict(size=(96, 54), depth=10, spp=4)


def assert_strip_equals_fresh(lib, s, bvh):
    """Both renderers on the updated scene against a fresh device scene of s.desc: fp32, unorm8 and the ray count."""
    cam = Camera.for_scene(s.desc, STRIP["size"])
    fresh = Scene(s.desc, 0, bvh, lib=lib)
    for cls in RENDERERS:
        assert_same_frame(frame(cls, s, cam, **STRIP), frame(cls, fresh, cam, **STRIP), cls.__name__)
    fresh.close()


@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH])
def test_full_size_atrium_device_refit_equals_host(devlib, scene_cache, bvh):
    sd = scene_cache("atrium", detail=4)
    assert sd.n_triangles > 1105 * 256
    dev = Scene(sd, 0, bvh, lib=devlib, updatable=True)
    host = Scene(sd, -1, bvh, lib=devlib, updatable=True)
    for k, u in enumerate(update_sequence(sd)):
        dev.update(**u)
        host.update(**u)
        tree = dev.tree()
        _tree_equal(tree, host.tree())
        _tables_equal(dev.shading_tables(), host.shading_tables(), lds=False)
        assert_model_words(devlib, tree)
        dev.check_bvh()
        assert_fresh_bounds(dev, bvh, devlib)
        if k == 0:  # the 35 degree spin
            assert_strip_equals_fresh(devlib, dev, bvh)
    dev.close()
    host.close()


def test_full_size_atrium_device_built_lbvh_is_refit_to_the_model(devlib, scene_cache):
    sd = scene_cache("atrium", detail=4)
    s = Scene(sd, 0, abi.RT_BVH_LBVH_GPU, lib=devlib, updatable=True)
    built = s.tree()
    assert built["built_by"] == abi.RT_BVH_LBVH_GPU
    for k, u in enumerate(update_sequence(sd)):
        s.update(**u)
        tree = s.tree()
        assert same_bits(tree["nodes"][:, 12:], built["nodes"][:, 12:]) and same_bits(tree["global_index"], built["global_index"])
        assert_model_words(devlib, tree)
        s.check_bvh()
        assert_fresh_bounds(s, abi.RT_BVH_LBVH, devlib)
        if k == 0:
            assert_strip_equals_fresh(devlib, s, abi.RT_BVH_LBVH_GPU)
    s.close()


# ---- 2. bounds attained by -0 and +0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ZERO_CASES, ids=[zero_case_id(c) for c in ZERO_CASES])
def test_device_reduction_keeps_the_first_signed_zero_bound(devlib, case):
    """The zeros placed in one wave, in two waves of a workgroup and in two workgroups, -0 first, +0 first and -0 alone, for the minimum and
    (on a scene <= 0 on that axis) the maximum: the device update's bounds bits, pad and tree are the host update's and the bounds and pad a
    fresh build's, reached by every kind of update from a scene whose bound is not zero."""
    axis = ZERO_CASES.index(case) % 3
    sd = signed_zero_scene(devlib, case, axis)
    side = "bounds_lo" if case[0] == "min" else "bounds_hi"
    for kind, start, updates in signed_zero_starts(sd, case, axis):
        dev = Scene(start, 0, abi.RT_BVH_SAH, lib=devlib, updatable=True)
        host = Scene(start, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
        assert dev.tree()[side][axis] != 0.0, kind
        for u in updates:
            dev.update(**u)
            host.update(**u)
            tree = dev.tree()
            assert tree[side][axis] == 0.0, kind
            _tree_equal(tree, host.tree())
            assert_fresh_bounds(dev, abi.RT_BVH_SAH, devlib)
            assert_model_words(devlib, tree)
        dev.close()
        host.close()


# ---- 3. every kind of update --------------------------------------------------------------------------------------------------------------
def kind_updates(sd):
    """(what, update) in turn: normals alone, positions alone, normals right after the positions (the buffer the positions swapped out
    stages them), transforms with positions, normals again, all three, positions alone."""
    rng = np.random.default_rng(sd.n_triangles + 7)

    def pos():
        return (sd.positions + rng.normal(scale=1e-2, size=sd.positions.shape)).astype(f32)

    def nrm():
        n = sd.normals + rng.normal(scale=0.2, size=sd.normals.shape)
        return (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)).astype(f32)

    return [("normals", dict(normals=nrm())), ("positions", dict(positions=pos())), ("normals after positions", dict(normals=nrm())),
            ("transforms+positions", dict(instances=spin_about_centre(sd, 20.0), positions=pos())),
            ("normals after transforms+positions", dict(normals=nrm())),
            ("transforms+positions+normals", dict(instances=spin_about_centre(sd, -15.0), positions=pos(), normals=nrm())),
            ("positions after all three", dict(positions=pos()))]


@pytest.mark.parametrize("name,kw", [("cornell", {}), ("atrium", {"detail": 1}), ("atrium_tilted", {"detail": 1})])
def test_every_update_kind_on_the_device(devlib, scene_cache, name, kw):
    sd = scene_cache(name, **kw)
    dev = Scene(sd, 0, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    host = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    if name == "atrium_tilted":
        assert dev.info().n_split_triangles > 0
    cam = Camera.for_scene(sd, (W, H))
    for what, u in kind_updates(sd):
        dev.update(**u)
        host.update(**u)
        _tree_equal(dev.tree(), host.tree())
        _tables_equal(dev.shading_tables(), host.shading_tables(), lds=False)
        fresh = Scene(dev.desc, 0, abi.RT_BVH_SAH, lib=devlib)
        org, d = rays(dev.desc, 3000, seed=5)
        assert_same_hits(dev, fresh, org, d)
        g, fg = dev.gbuffer(cam), fresh.gbuffer(cam)
        for k in ("albedo", "normal", "position"):
            assert same_bits(g[k], fg[k]), (what, k)
        if name == "cornell":
            for cls in RENDERERS:
                assert_same_frame(frame(cls, dev, cam), frame(cls, fresh, cam), f"{what}: {cls.__name__}")
        fresh.close()
    dev.close()
    host.close()


# ---- 4. round trips -----------------------------------------------------------------------------------------------------------------------
# the device image at its edges: a record array that ends in a leaf of one record (the whole-leaf step's 80-byte read runs into the array's
# tail), and a tree of one triangle (the device builder refuses it and the host builds)
IMAGE_EDGES = [(abi.RT_BVH_SAH, "odd_tail", {}), (abi.RT_BVH_LBVH, "odd_tail", {}), (abi.RT_BVH_LBVH_GPU, "one_triangle", {})]


@pytest.mark.parametrize("bvh,name,kw", _exact_union_builders() + [(abi.RT_BVH_LBVH_GPU, "atrium", {"detail": 1})] + IMAGE_EDGES)
def test_device_round_trips_give_the_built_tree_back(devlib, scene_cache, bvh, name, kw):
    """Trees whose child boxes are exact subtree unions: an update with the scene's own transforms, positions and normals, and D -> D' -> D,
    give all 16 words of every node back, and the SAH cost within rel 1e-9."""
    sd = get_scene(scene_cache, name, kw)
    s = Scene(sd, 0, bvh, lib=devlib, updatable=True)
    assert s.info().n_split_triangles == 0
    built, tables, cost = s.tree(), s.shading_tables(), s.info().sah_cost
    if (bvh, name, kw) in IMAGE_EDGES:
        assert last_leaf_count(built) == 1
        assert name != "one_triangle" or built["built_by"] != abi.RT_BVH_LBVH_GPU
    own = dict(instances=(sd.transforms, sd.normal_mats), positions=sd.positions, normals=sd.normals)

    def assert_built():
        _tree_equal(s.tree(), built)
        _tables_equal(s.shading_tables(), tables)
        if name != "one_triangle":  # (a tree of one leaf is built with the cost of its records alone, emit_tree; a refit counts the root's step too)
            assert s.info().sah_cost == pytest.approx(cost, rel=1e-9)
        s.check_bvh()

    s.update(**own)
    assert_built()
    seq = update_sequence(sd)
    s.update(**seq[0])
    s.update(**seq[3])
    assert not same_bits(s.tree()["nodes"], built["nodes"])
    s.update(**own)
    assert_built()
    s.close()


# ---- 5. refusals of non-finite vertices -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["transform", "positions"])
@pytest.mark.parametrize("value", [math.nan, math.inf, -math.inf], ids=["nan", "+inf", "-inf"])
def test_device_refuses_non_finite_vertices(devlib, scene_cache, where, value):
    """A NaN or an inf in a transform or in the positions: RT_ERR_INVALID, "non-finite", and the tree, tables, frame and closest hits as they
    were. The refusal restores the scratch world vertices the lazy host copy reads (the update before it left the host copy stale), and
    the next update still equals the host path."""
    sd = scene_cache("cornell")
    cam = Camera.for_scene(sd, (W, H))
    dev = Scene(sd, 0, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    host = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    u = update_sequence(sd)[0]
    dev.update(**u)
    host.update(**u)
    r = MegakernelRenderer(dev, (W, H), DEPTH, SPP)
    before = r.render_frame(cam)
    org, d = rays(dev.desc, 2000, seed=9)
    hits = dev.intersect(org, d)
    if where == "transform":
        xf = np.array(dev.desc.transforms, f32, copy=True)
        xf[int(sd.tri_instance[0]), 5] = value
        bad = dict(instances=(xf, dev.desc.normal_mats))
    else:
        pos = dev.desc.positions.copy()
        pos[int(sd.indices[3, 0]), 2] = value
        bad = dict(positions=pos)
    for s in (dev, host):
        status, msg = _status(s, **bad)
        assert status == abi.RT_ERR_INVALID and "non-finite" in msg, msg
    _tree_equal(dev.tree(), host.tree())
    _tables_equal(dev.shading_tables(), host.shading_tables(), lds=False)
    assert_same_frame(r.render_frame(cam), before)
    for a, b in zip(dev.intersect(org, d), hits):
        assert same_bits(a, b)
    u = dict(instances=spin_about_centre(sd, 10.0), positions=sd.positions)
    dev.update(**u)
    host.update(**u)
    _tree_equal(dev.tree(), host.tree())
    _tables_equal(dev.shading_tables(), host.shading_tables(), lds=False)
    fresh = Scene(dev.desc, 0, abi.RT_BVH_SAH, lib=devlib)
    assert_same_frame(r.render_frame(cam), frame(MegakernelRenderer, fresh, cam))
    fresh.close()
    r.close()
    dev.close()
    host.close()


# ---- 6. shading tables across their limits ------------------------------------------------------------------------------------------------
def table_updates(sd):
    """A rotation of its own per instance (a row per instance: past kLdsNm), one rotation shared by all (the rows shrink back to the scene's
    patterns, in new slots), the original transforms."""
    rng = np.random.default_rng(41)
    xf0, nm0 = sd.transforms, sd.normal_mats
    n = xf0.shape[0]
    own = np.stack([scenes.mat4_mul(xf0[i], scenes.mat4_from_quat(scenes.quat_axis_angle(rng.normal(size=3), float(rng.uniform(0.1, 0.5)))))
                    for i in range(n)])
    shared_rot = scenes.mat4_from_quat(scenes.quat_axis_angle((1.0, 2.0, 0.5), 0.3))
    shared = np.stack([scenes.mat4_mul(xf0[i], shared_rot) for i in range(n)])
    nms = [np.stack([scenes.normal_matrix(m) for m in x]) for x in (own, shared)]
    return [("own rotations", (own, nms[0])), ("shared rotation", (shared, nms[1])), ("original", (xf0, nm0))]


def assert_high_materials_read(oracle, s):
    """test_gpu_parity's rt_probe_scatter reads of materials 24, 4095 and 4096 (where the scene has them) on the updated scene."""
    sd = s.desc
    osc = oracle.OracleScene(sd)
    rng = np.random.default_rng(24)
    n = 1024
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)  # noqa: E731
    dirs, nrm = unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3)))
    uv = rng.uniform(-3, 3, (n, 2)).astype(f32)
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for m in sorted({0, 24, 4095, 4096, len(sd.materials) - 1} & set(range(len(sd.materials)))):
        for a, b in zip(s.scatter(m, dirs, nrm, uv, seeds), osc.scatter(m, dirs, nrm, uv, seeds)):
            np.testing.assert_array_equal(a, b, err_msg=f"material {m}")


@pytest.mark.parametrize("case,kw,tables", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_shading_tables_follow_updates_across_their_limits(devlib, scene_cache, oracle, case, kw, tables):
    sd = scene_cache("tables", **kw)
    dev = Scene(sd, 0, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    host = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    cam = Camera.for_scene(sd, (W, H))
    n_inst = sd.transforms.shape[0]
    for what, inst in table_updates(sd):
        dev.update(instances=inst)
        host.update(instances=inst)
        t = dev.shading_tables()
        fresh = Scene(dev.desc, 0, abi.RT_BVH_SAH, lib=devlib)
        _tables_equal(t, fresh.shading_tables())
        _tables_equal(t, host.shading_tables(), lds=False)
        assert t["packed_mat"] == tables[0], what
        if t["packed_mat"]:
            rows = {"own rotations": n_inst}.get(what, kw["n_rows"])
            assert t["rows"].shape[0] == rows and t["lds_nm"] == min(rows, 8), what
        else:
            assert t["rows"].shape[0] == n_inst and t["lds_nm"] == 0, what
        for cls in RENDERERS:
            assert_same_frame(frame(cls, dev, cam, spp=2), frame(cls, fresh, cam, spp=2), f"{case}, {what}: {cls.__name__}")
        if kw["n_mats"] > 24:
            assert_high_materials_read(oracle, dev)
        fresh.close()
    dev.close()
    host.close()


# ---- 7. deep host-built trees ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH])
def test_deep_host_built_tree_is_refit_on_the_device(devlib, bvh):
    sd = chain_scene()
    dev = Scene(sd, 0, bvh, lib=devlib, updatable=True)
    host = Scene(sd, -1, bvh, lib=devlib, updatable=True)
    built = dev.tree()
    if bvh == abi.RT_BVH_LBVH:
        assert built["built_by"] == abi.RT_BVH_MEDIAN_INTERNAL
    for u in update_sequence(sd):
        dev.update(**u)
        host.update(**u)
        tree = dev.tree()
        _tree_equal(tree, host.tree())
        assert_model_words(devlib, tree)
        dev.check_bvh()
        fresh = Scene(dev.desc, 0, bvh, lib=devlib)
        org, d = rays(dev.desc, 3000, seed=13)
        assert_same_hits(dev, fresh, org, d)
        fresh.close()
    dev.close()
    host.close()


# ---- 8. a creation that fails part-way ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH_GPU], ids=["sah", "lbvh_gpu"])
@pytest.mark.parametrize("name", ["cornell", "empty"])
def test_failed_scene_creation_leaves_nothing_behind(devlib, scene_cache, monkeypatch, name, bvh):
    """RT_INJECT_ALLOC_FAILURE=k (developer build) fails the k-th allocation of a scene creation as out of memory, without calling the
    runtime: every k up to the number of allocations gives RT_ERR_OOM and a scene that frees what it held by then. The hook covers all of
    them: the image's seven arrays and the query cursors, the updatable state's twelve device arrays (eleven in the empty scene, which keeps
    no previous vertices) and its pinned reduction words. Afterwards a creation accounts for the same device memory as one made before any
    failure, its tree passes the check, and it follows an update as that twin does."""
    sd = scene_cache(name)

    def make():
        return Scene(sd, 0, bvh, lib=devlib, updatable=True, keep_previous=True)

    twin = make()
    failures = 0
    for k in range(1, 65):
        monkeypatch.setenv("RT_INJECT_ALLOC_FAILURE", str(k))
        try:
            make().close()  # (k is past the creation's last allocation)
            break
        except abi.RtError as e:
            assert e.status == abi.RT_ERR_OOM, (k, e)
            failures += 1
        finally:
            monkeypatch.delenv("RT_INJECT_ALLOC_FAILURE")
    else:
        pytest.fail("scene creation still fails at k = 64")
    print(f"{name}: {failures} allocations")
    assert failures == (7 + 1 + 12 + 1 if sd.n_triangles else 7 + 1 + 11 + 1)
    assert failures >= 19 or not sd.n_triangles
    s = make()
    assert s.info().device_bytes == twin.info().device_bytes
    s.check_bvh()
    turn = dict(instances=spin_about_centre(sd, 25.0))
    s.update(**turn)
    twin.update(**turn)
    _tree_equal(s.tree(), twin.tree())
    _tables_equal(s.shading_tables(), twin.shading_tables())
    s.check_bvh()
    s.close()
    twin.close()
