"""Dynamic scenes on the host (no GPU): rt_scene_update of host-only scenes (device < 0), the CPU reference of the device refit.

The contract (include/rt_mi355x.h): an updatable scene made from D, after rt_scene_update(S, U), behaves as rt_scene_create(D') would, D' being
D with U applied — closest hits, bounds, padding, shading tables — and only its tree differs: the topology is kept and the boxes are refit.
"""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Scene

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
K_CHILD_EMPTY = 0x80000000


# ---- updates ---------------------------------------------------------------------------------------------------------------------------
def spin_about_centre(sd, deg: float, inst=None, centre=None) -> tuple[np.ndarray, np.ndarray]:
    """Every instance (or those listed) rotated by `deg` about the vertical axis through `centre` (default: the centre of the scene's world
    bounds)."""
    if centre is None:
        wt = sd.world_triangles().reshape(-1, 3)
        centre = (wt.min(0) + wt.max(0)) / 2 if len(wt) else np.zeros(3)
    c = np.asarray(centre, np.float64)
    r = scenes.mat4_mul(scenes.mat4_translate(c), scenes.mat4_mul(scenes.mat4_from_quat(scenes.quat_axis_angle((0, 1, 0), math.radians(deg))),
                                                                     scenes.mat4_translate(-c)))
    xf = np.array(sd.transforms, f32, copy=True)
    nm = np.array(sd.normal_mats, f32, copy=True)
    for i in range(xf.shape[0]) if inst is None else inst:
        xf[i] = scenes.mat4_mul(r, sd.transforms[i])
        nm[i] = scenes.normal_matrix(xf[i])
    return xf, nm


def update_sequence(sd):
    """Successive updates (kwargs of Scene.update), each applied to the result of the previous: a rotation of everything, a mirror on one
    instance with a translation of another, zero scale on one instance with a large translation of another, and an edit of the vertices."""
    out = []
    xf, nm = spin_about_centre(sd, 35.0)
    out.append(dict(instances=(xf, nm)))
    xf2, nm2 = xf.copy(), nm.copy()
    mirror = scenes.mat4_scale((-1.0, 1.0, 1.0))
    xf2[0] = scenes.mat4_mul(xf[0], mirror)
    nm2[0] = scenes.normal_matrix(xf2[0])
    if xf.shape[0] > 1:
        xf2[-1] = scenes.mat4_mul(scenes.mat4_translate((0.25, -0.5, 0.125)), xf[-1])
        nm2[-1] = scenes.normal_matrix(xf2[-1])
    out.append(dict(instances=(xf2, nm2)))
    xf3, nm3 = xf2.copy(), nm2.copy()
    xf3[-1] = scenes.mat4_mul(xf2[-1], scenes.mat4_scale((0.0, 0.0, 0.0)))  # (its normal matrix is left as it was: any fp32 pattern is data)
    xf3[0] = scenes.mat4_mul(scenes.mat4_translate((3.0e3, -1.5e3, 750.0)), xf2[0])
    nm3[0] = scenes.normal_matrix(xf3[0])
    out.append(dict(instances=(xf3, nm3)))
    rng = np.random.default_rng(sd.n_triangles)
    pos = sd.positions + rng.normal(scale=1e-2, size=sd.positions.shape).astype(f32)
    nrm = sd.normals + rng.normal(scale=0.2, size=sd.normals.shape).astype(f32)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), f32(1e-6))
    out.append(dict(positions=pos.astype(f32), normals=nrm.astype(f32)))
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def _box_tri(lo, hi):
    """A triangle whose box is exactly [lo, hi]."""
    return [[lo[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], hi[2]]]


def chain_scene(m: int = 63, dups: int = 40):
    """Tiny triangles on the Morton cells of keys 0 (dups + 1 times), 2^0 .. 2^(m-1) and the far corner of [0, 1]^3: the host LBVH is a
    chain too deep for the traversal stack and falls back to the balanced tree (RT_BVH_MEDIAN_INTERNAL). Two instances (the chain, the
    duplicates), so that an update can move them apart."""
    h = 2.0 ** -24
    chain = [_box_tri((1 - 2 * h,) * 3, (1, 1, 1))]
    for i in range(m):
        q = [0, 0, 0]
        q[2 - i % 3] = 1 << (i // 3)
        c = [(v + 0.5) * 2.0 ** -21 for v in q]
        chain.append(_box_tri([v - h for v in c], [v + h for v in c]))
    sb = scenes.SceneBuilder("chain")
    mat = sb.add_material(scenes.Material(abi.RT_MAT_DIFFUSE, (0.6, 0.5, 0.4)))
    for tris in (chain, [_box_tri((0, 0, 0), (2 * h,) * 3)] * (dups + 1)):
        pos = np.asarray(tris, f32).reshape(-1, 3)
        nrm = np.tile(np.array([[0, 0, 1]], f32), (pos.shape[0], 1))
        sb.add_instance(sb.add_mesh(pos, nrm, np.zeros((pos.shape[0], 2), f32), np.arange(pos.shape[0], dtype=np.uint32)), mat)
    sb.camera = scenes.CameraPose((0.5, 0.5, 3.0), (0, 0, -1), 1.2)
    return sb.build()


ZERO_TRIS = 700  # three reduction workgroups of 256 triangles (k_upd_transform: one thread per triangle, waves of 64)
ZERO_PLACES = {"wave": (10, 41), "waves": (10, 200), "workgroups": (10, 310)}  # the triangles of the two zeros (slots 3t + k)
ZERO_CASES = [(bound, order, place) for bound in ("min", "max") for order in ("neg_first", "pos_first") for place in ZERO_PLACES] + \
             [("min", "neg_only", "workgroups"), ("max", "neg_only", "workgroups")]
ZERO_MIX = -0.0  # off-diagonals and translation of the scene's transform: x * 1 + (-0 * y) + (-0 * z) + (-0) is x, sign of a zero included


def _zero_transform():
    """Identity with -0 off-diagonals and translation: world = object, bit for bit, while every other coordinate is positive."""
    m = np.full(16, ZERO_MIX, f32)
    m[0] = m[5] = m[10] = m[15] = 1.0
    m[3] = m[7] = m[11] = 0.0
    return m


def signed_zero_scene(lib, case, axis):
    """ZERO_TRIS triangles whose world coordinates on `axis` are all >= 0 (case[0] "min") or all <= 0 ("max"), the bound attained at exactly
    0 by two vertices at the slots ZERO_PLACES[case[2]] names: -0 then +0 ("neg_first"), +0 then -0 ("pos_first"), or -0 alone ("neg_only").
    Every other coordinate is positive, so the transform keeps the zeros' signs. The host std::min / std::max keep the first of equal values:
    the bound is the first zero's bits. Asserted here on a fresh host build's world vertices, else a test of it checks nothing."""
    bound, order, place = case
    rng = np.random.default_rng(17 + axis)
    pos = rng.uniform(1.0, 2.0, (ZERO_TRIS, 3, 3)).astype(f32)
    side = f32(1.0) if bound == "min" else f32(-1.0)
    pos[:, :, axis] = side * rng.uniform(0.5, 1.5, (ZERO_TRIS, 3)).astype(f32)
    first, second = ZERO_PLACES[place]
    zeros = {"neg_first": (-0.0, 0.0), "pos_first": (0.0, -0.0), "neg_only": (-0.0, None)}[order]
    slots = []
    for t, k, z in ((first, 1, zeros[0]), (second, 2, zeros[1])):
        if z is not None:
            pos[t, k, axis] = z
            slots.append((3 * t + k, z))
    sb = scenes.SceneBuilder(f"zero_{bound}_{order}_{place}_{axis}")
    mat = sb.add_material(scenes.Material(abi.RT_MAT_DIFFUSE, (0.6, 0.5, 0.4)))
    p = pos.reshape(-1, 3)
    nrm = np.tile(np.array([[0, 0, 1]], f32), (p.shape[0], 1))
    sb.add_instance(sb.add_mesh(p, nrm, np.zeros((p.shape[0], 2), f32), np.arange(p.shape[0], dtype=np.uint32)), mat, _zero_transform())
    sb.camera = scenes.CameraPose((1.5, 1.5, 6.0), (0, 0, -1), 1.2)
    sd = sb.build()
    s = Scene(sd, -1, abi.RT_BVH_SAH, lib=lib)
    tree = s.tree()
    s.close()
    w = tree["wverts"].reshape(-1, 3)[:, axis]
    assert same_bits(w, pos.reshape(-1, 3)[:, axis]), "the transform changed a coordinate"
    at_zero = np.nonzero(w == 0.0)[0]
    assert [int(v) for v in at_zero] == [v for v, _ in slots]
    for v, z in slots:
        assert np.signbit(w[v]) == np.signbit(z), (v, z)
    want = f32(slots[0][1])
    got = tree["bounds_lo" if bound == "min" else "bounds_hi"][axis]
    assert got == 0.0 and np.signbit(got) == np.signbit(want), "the bound is not the first zero"
    return sd


def signed_zero_starts(sd, case, axis):
    """(kind, start description, updates) that reach sd from a scene whose bound on `axis` is not zero, through every kind of update: the
    transform alone, the positions alone, both, all three, and a normals-only call right after a positions call (the device then stages the
    normals in the buffer the positions call swapped out). The reduction of the update, not the build, makes the zero bound."""
    sign = 1.0 if case[0] == "min" else -1.0
    shift = [0.0, 0.0, 0.0]
    shift[axis] = sign
    xf = np.array(sd.transforms, f32, copy=True)
    moved = xf.copy()
    moved[0] = scenes.mat4_mul(scenes.mat4_translate(shift), xf[0])
    pos = sd.positions.copy()
    pos[:, axis] += f32(0.25 * sign)
    nrm = np.tile(np.array([[0, 1, 0]], f32), (sd.positions.shape[0], 1))
    own = (sd.transforms, sd.normal_mats)
    return [
        ("transforms", sd.updated(instances=(moved, sd.normal_mats)), [dict(instances=own)]),
        ("positions", sd.updated(positions=pos), [dict(positions=sd.positions)]),
        ("transforms+positions", sd.updated(instances=(moved, sd.normal_mats), positions=pos), [dict(instances=own, positions=sd.positions)]),
        ("transforms+positions+normals", sd.updated(instances=(moved, sd.normal_mats), positions=pos, normals=nrm),
         [dict(instances=own, positions=sd.positions, normals=sd.normals)]),
        ("positions, then normals", sd.updated(positions=pos, normals=nrm), [dict(positions=sd.positions), dict(normals=sd.normals)]),
    ]


def zero_case_id(case):
    return "-".join(case)


SCENES = [("cornell", {}), ("table", {}), ("atrium", {"detail": 1}), ("atrium", {"detail": 2}), ("voxel", {"detail": 1}),
          ("atrium_tilted", {"detail": 1})]


def soup_scene(name, tris):
    """A one-instance scene of the given (n, 3, 3) triangles."""
    sb = scenes.SceneBuilder(name)
    mat = sb.add_material(scenes.Material(abi.RT_MAT_DIFFUSE, (0.6, 0.5, 0.4)))
    pos = np.asarray(tris, f32).reshape(-1, 3)
    nrm = np.tile(np.array([[0, 0, 1]], f32), (pos.shape[0], 1))
    sb.add_instance(sb.add_mesh(pos, nrm, np.zeros((pos.shape[0], 2), f32), np.arange(pos.shape[0], dtype=np.uint32)), mat)
    sb.camera = scenes.CameraPose((0.5, 0.5, 3.0), (0, 0, -1), 1.2)
    return sb.build()


def last_leaf_count(tree):
    """The number of records in the leaf that ends the leaf-ordered record array."""
    words = tree["nodes"][:, 12:].ravel()
    codes = ~words[(words & K_CHILD_EMPTY != 0) & (words != K_CHILD_EMPTY)]
    first, count = codes >> 2, (codes & 3) + 1
    assert int((first + count).max()) == len(tree["global_index"])
    return int(count[np.argmax(first)])


def get_scene(scene_cache, name, kw):
    if name == "table":
        return scene_cache("tables", n_mats=25, n_rows=6)
    if name == "one_triangle":  # (the device builder refuses it: the host builds the tree)
        return soup_scene(name, [[[0, 0, 0], [1, 0, 0], [0, 1, 0.5]]])
    if name == "odd_tail":  # three triangles, two of them close: the last leaf of the record array holds one record
        return soup_scene(name, [_box_tri((x, 0, 0), (x + 0.5, 1, 1)) for x in (0.0, 1.0, 10.0)])
    return scene_cache(name, **kw)


# ---- readers ----------------------------------------------------------------------------------------------------------------------------
def rays(sd, n=1500, seed=3):
    rng = np.random.default_rng(seed)
    wt = sd.world_triangles().reshape(-1, 3)
    lo, hi = wt.min(0), wt.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    org = (lo - 0.2 * ext + rng.uniform(0, 1, (n, 3)) * 1.4 * ext).astype(f32)
    tgt = wt[rng.integers(0, len(wt), n)]
    d = (tgt - org) + rng.normal(scale=0.05, size=(n, 3)) * ext
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    return org, d


def closest_hits(scene, org, d):
    n = org.shape[0]
    t, tri = np.zeros(n, f32), np.zeros(n, np.uint32)
    nv, nt = C.c_uint64(), C.c_uint64()
    abi.check(scene._lib.rt_scene_count_visits(scene.h, n, abi.fptr(org), abi.fptr(d), 0, C.byref(nv), C.byref(nt), abi.fptr(t), abi.u32ptr(tri)),
              scene._lib)
    return t, tri


def quantise(lib, nk, klo, khi):
    nk = np.ascontiguousarray(nk, np.int32)
    klo, khi = np.ascontiguousarray(klo, f32), np.ascontiguousarray(khi, f32)
    m = nk.shape[0]
    out = np.zeros((m, 16), np.uint32)
    ok = np.zeros(m, np.uint8)
    abi.check(lib.rt_dev_quantise_node(m, abi.i32ptr(nk), abi.fptr(klo), abi.fptr(khi), out.ctypes.data_as(C.c_void_p), abi.u8ptr(ok)), lib)
    return out, ok.astype(bool)


def model_node_words(lib, tree):
    """Words 0..11 every node must hold: rt_dev_quantise_node on the padded exact boxes of its children, recomputed here from the world
    vertices (a leaf child: the union of its triangles' whole boxes; an inner child: the union of its own children)."""
    nodes, gi, wv, pad = tree["nodes"], tree["global_index"], tree["wverts"], tree["pad"]
    tri_lo, tri_hi = wv.min(1), wv.max(1)  # (T, 3) fp32, exact
    n = nodes.shape[0]
    box_lo, box_hi = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    nk = np.zeros(n, np.int32)
    klo, khi = np.zeros((n, 4, 3), f32), np.zeros((n, 4, 3), f32)
    child = nodes[:, 12:16].view(np.int32)
    for i in range(n - 1, -1, -1):  # children are emitted after their parents
        los, his = [], []
        for c in child[i]:
            if c == np.int32(-2 ** 31):
                break
            if c >= 0:
                assert c > i
                los.append(box_lo[c]), his.append(box_hi[c])
            else:
                code = int(~c) & 0xFFFFFFFF
                recs = gi[code >> 2: (code >> 2) + (code & 3) + 1]
                los.append(tri_lo[recs].min(0)), his.append(tri_hi[recs].max(0))
        k = nk[i] = len(los)
        if k:
            klo[i, :k] = np.stack(los) - pad
            khi[i, :k] = np.stack(his) + pad
            box_lo[i], box_hi[i] = np.min(los, 0), np.max(his, 0)
    live = nk > 0
    words, ok = quantise(lib, nk[live], klo[live], khi[live])
    assert ok.all()
    out = np.zeros((n, 12), np.uint32)
    out[live] = words[:, :12]
    return out, live


def _mt_double(o, d, w):
    """Moller-Trumbore in double as rt_scene_count_visits runs it (scene_check.cpp: count_visits): t, or inf on a miss."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    v0 = w[0]
    e1, e2 = (f32(w[1] - w[0])).astype(np.float64), (f32(w[2] - w[0])).astype(np.float64)
    p = np.cross(d, e2)
    det = e1 @ p
    if det == 0.0:
        return np.inf
    tv = o - v0
    u = (tv @ p) / det
    q = np.cross(tv, e1)
    v = (d @ q) / det
    if u < 0.0 or v < 0.0 or u + v > 1.0:
        return np.inf
    return (e2 @ q) / det


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _tree_equal(a, b):
    for k in ("nodes", "global_index", "wverts", "pad", "bounds_lo", "bounds_hi", "stack_need", "built_by"):
        assert same_bits(np.asarray(a[k]), np.asarray(b[k])), k


def _tables_equal(a, b, lds=True):
    for k in ("packed_mat",) + (("lds_nm", "lds_mats") if lds else ()):
        assert a[k] == b[k], k
    assert same_bits(a["rows"], b["rows"]) and same_bits(a["words"], b["words"])


def check_against_fresh(devlib, s, bvh, built, org, d):
    """s (updated) against a fresh host scene of s.desc: structure, closest hits, world vertices / bounds / pad, node words, tables."""
    s.check_bvh()
    fresh = Scene(s.desc, -1, bvh, lib=devlib)
    try:
        (t, tri), (ft, ftri) = closest_hits(s, org, d), closest_hits(fresh, org, d)
        tree, ftree = s.tree(), fresh.tree()
        assert same_bits(t, ft)
        ties = np.nonzero(tri != ftri)[0]
        if len(ties):  # the host walk's double-precision test can leave a tie between two triangles hit at one fp32 t to the tree's order
            tv = ftree["wverts"].astype(np.float64)
            for r in ties:
                for k in (tri[r], ftri[r]):
                    assert k != 0xFFFFFFFF and abs(_mt_double(org[r], d[r], tv[k]) - float(t[r])) <= 2 * float(np.spacing(t[r])), (r, k)
            assert len(ties) < len(t) // 50
        assert same_bits(tree["nodes"][:, 12:16], built["nodes"][:, 12:16]), "child words changed"
        assert same_bits(tree["global_index"], built["global_index"]), "leaf record order changed"
        assert same_bits(tree["wverts"], ftree["wverts"])
        assert same_bits(tree["bounds_lo"], ftree["bounds_lo"]) and same_bits(tree["bounds_hi"], ftree["bounds_hi"])
        assert same_bits(tree["pad"], ftree["pad"])
        words, live = model_node_words(devlib, tree)
        assert same_bits(tree["nodes"][live, :12], words[live])
        ta, tb = s.shading_tables(), fresh.shading_tables()
        for k in ("packed_mat", "lds_nm", "lds_mats"):
            assert ta[k] == tb[k], k
        assert same_bits(ta["rows"], tb["rows"]) and same_bits(ta["words"], tb["words"])
        info, finfo = s.info(), fresh.info()
        assert list(info.bounds_lo) == list(finfo.bounds_lo) and list(info.bounds_hi) == list(finfo.bounds_hi)
        assert np.isfinite(info.sah_cost) and info.sah_cost >= 1.0
    finally:
        fresh.close()


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH])
@pytest.mark.parametrize("name,kw", SCENES)
def test_host_update_behaves_as_a_fresh_build(devlib, scene_cache, name, kw, bvh):
    sd = get_scene(scene_cache, name, kw)
    s = Scene(sd, -1, bvh, lib=devlib, updatable=True)
    built = s.tree()
    org, d = rays(sd)
    for u in update_sequence(sd):
        st = s.update(**u)
        assert st.device_ms == 0.0 and st.launches == 0 and st.refit_nodes == built["nodes"].shape[0]
        check_against_fresh(devlib, s, bvh, built, org, d)
    s.close()


def test_median_fallback_tree_is_refit(devlib):
    sd = chain_scene()
    s = Scene(sd, -1, abi.RT_BVH_LBVH, lib=devlib, updatable=True)
    built = s.tree()
    assert built["built_by"] == abi.RT_BVH_MEDIAN_INTERNAL
    org, d = rays(sd)
    for u in update_sequence(sd):
        s.update(**u)
        check_against_fresh(devlib, s, abi.RT_BVH_LBVH, built, org, d)
    s.close()


def _exact_union_builders():
    return [(abi.RT_BVH_LBVH, "atrium", {"detail": 1}), (abi.RT_BVH_SAH, "atrium", {"detail": 2}), (abi.RT_BVH_SAH, "cornell", {}),
            (abi.RT_BVH_LBVH, "voxel", {"detail": 1})]


@pytest.mark.parametrize("bvh,name,kw", _exact_union_builders())
def test_unchanged_update_reproduces_the_built_tree(devlib, scene_cache, bvh, name, kw):
    """Trees whose child boxes are exact subtree unions (every builder without pre-split triangles): an update with the scene's own transforms
    and vertices gives the built tree back bit for bit, all 16 words of every node, and the same SAH cost."""
    sd = get_scene(scene_cache, name, kw)
    s = Scene(sd, -1, bvh, lib=devlib, updatable=True)
    assert s.info().n_split_triangles == 0
    built, cost = s.tree(), s.info().sah_cost
    s.update(instances=(sd.transforms, sd.normal_mats), positions=sd.positions, normals=sd.normals)
    tree = s.tree()
    assert same_bits(tree["nodes"], built["nodes"]) and same_bits(tree["global_index"], built["global_index"])
    assert same_bits(tree["wverts"], built["wverts"]) and same_bits(tree["pad"], built["pad"])
    assert s.info().sah_cost == pytest.approx(cost, rel=1e-9)
    s.check_bvh()
    s.close()


def test_presplit_tree_bounds_whole_triangles(devlib, scene_cache):
    """A pre-split SAH tree (the tilted atrium): after an update with unchanged transforms every leaf record bounds its whole triangle
    (check_bvh on the reset record boxes) and the closest hits are those of the fresh build."""
    sd = scene_cache("atrium_tilted", detail=1)
    s = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    assert s.info().n_split_triangles > 0
    built = s.tree()
    s.update(instances=(sd.transforms, sd.normal_mats))
    org, d = rays(sd)
    check_against_fresh(devlib, s, abi.RT_BVH_SAH, built, org, d)
    s.close()


@pytest.mark.parametrize("case", ZERO_CASES, ids=[zero_case_id(c) for c in ZERO_CASES])
def test_host_update_keeps_the_first_signed_zero_bound(devlib, case):
    """Bounds attained at 0 by -0 and +0 (and by -0 alone): the host update, reached by every kind of update from non-zero bounds, gives the
    bounds bits of a fresh build, which are the first zero's in scene order."""
    axis = ZERO_CASES.index(case) % 3
    sd = signed_zero_scene(devlib, case, axis)
    fresh = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib)
    ftree = fresh.tree()
    fresh.close()
    for kind, start, updates in signed_zero_starts(sd, case, axis):
        s = Scene(start, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
        assert s.tree()["bounds_lo" if case[0] == "min" else "bounds_hi"][axis] != 0.0, kind
        for u in updates:
            s.update(**u)
        tree = s.tree()
        for k in ("wverts", "pad", "bounds_lo", "bounds_hi"):
            assert same_bits(tree[k], ftree[k]), (kind, k)
        s.check_bvh()
        s.close()


def _status(s, **u):
    try:
        s.update(**u)
    except abi.RtError as e:
        return e.status, str(e)
    return abi.RT_OK, ""


def test_update_refusals(devlib, scene_cache):
    sd = scene_cache("cornell")
    plain = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib)
    assert _status(plain, instances=(sd.transforms, sd.normal_mats))[0] == abi.RT_ERR_INVALID
    plain.close()
    s = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    before = s.tree()
    assert _status(s, instances=(sd.transforms[:-1], sd.normal_mats[:-1]))[0] == abi.RT_ERR_INVALID  # wrong count
    assert _status(s, positions=sd.positions[:-1])[0] == abi.RT_ERR_INVALID
    # a changed material, NULL with a count
    u = abi.rt_scene_update_desc()
    insts = sd.to_c().instances
    u.n_instances, u.instances = sd.transforms.shape[0], insts
    insts[0].material = (insts[0].material + 1) % len(sd.materials)
    assert devlib.rt_scene_update(s.h, C.byref(u), None) == abi.RT_ERR_INVALID and b"material" in devlib.rt_last_error()
    u = abi.rt_scene_update_desc()
    u.n_instances = sd.transforms.shape[0]
    assert devlib.rt_scene_update(s.h, C.byref(u), None) == abi.RT_ERR_INVALID
    u = abi.rt_scene_update_desc()
    u.n_vertices = sd.positions.shape[0]
    assert devlib.rt_scene_update(s.h, C.byref(u), None) == abi.RT_ERR_INVALID
    assert devlib.rt_scene_update(s.h, None, None) == abi.RT_ERR_INVALID
    # world vertices beyond fp32 / not finite: refused with rt_scene_create's test, the scene unchanged
    for scale in (3.0e38, float("nan")):
        xf = np.array(sd.transforms, f32, copy=True)
        xf[0] = scenes.mat4_mul(scenes.mat4_scale((scale, 1.0, 1.0)), xf[0])
        xf[1] = scenes.mat4_mul(scenes.mat4_scale((-scale, 1.0, 1.0)), xf[1])
        status, msg = _status(s, instances=(xf, sd.normal_mats))
        assert status == abi.RT_ERR_INVALID and ("overflows fp32" in msg or "non-finite" in msg), msg
        after = s.tree()
        for k in ("nodes", "global_index", "wverts", "pad", "bounds_lo", "bounds_hi"):
            assert same_bits(after[k], before[k]), k
        s.check_bvh()
    assert s.desc is sd
    # and the scene still updates
    xf, nm = spin_about_centre(sd, 10.0)
    s.update(instances=(xf, nm))
    org, d = rays(sd)
    check_against_fresh(devlib, s, abi.RT_BVH_SAH, before, org, d)
    s.close()


def test_unknown_scene_flags_are_refused(rtlib, scene_cache):
    sd = scene_cache("cornell")
    c = sd.to_c()
    h = C.c_void_p()
    assert rtlib.rt_scene_create_ex(C.byref(c), -1, abi.RT_BVH_SAH, 2, C.byref(h)) == abi.RT_ERR_INVALID
    assert rtlib.rt_scene_create_ex(C.byref(c), -1, abi.RT_BVH_SAH, abi.RT_SCENE_UPDATABLE, C.byref(h)) == abi.RT_OK
    rtlib.rt_scene_destroy(h)


def test_update_of_an_empty_scene(devlib, scene_cache):
    sd = scene_cache("empty")
    s = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    s.update(instances=(sd.transforms, sd.normal_mats))
    s.check_bvh()
    s.close()


def test_update_structs_match_header(tmp_path):
    names = ["rt_scene_update_desc", "rt_update_stats"]
    fields = {"rt_scene_update_desc": ["n_instances", "instances", "n_vertices", "positions", "normals"],
              "rt_update_stats": ["device_ms", "launches", "refit_nodes"]}
    src = tmp_path / "sz.c"
    body = "".join(f'printf("%zu\\n", sizeof({n}));' + "".join(f'printf("%zu\\n", offsetof({n}, {f}));' for f in fields[n]) for n in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){' + body + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for n in names:
        t = getattr(abi, n)
        want += [C.sizeof(t)] + [getattr(t, f).offset for f in fields[n]]
    assert vals == want
    assert "RT_SCENE_UPDATABLE 1u" in (REPO / "include" / "rt_mi355x.h").read_text() and abi.RT_SCENE_UPDATABLE == 1
