"""What the occlusion-gather tests share (tests/test_occlusion.py: the host statement; tests/test_gpu_occlusion.py: the device): the
contract of include/rt_mi355x.h: rt_occlusion_query in numpy fp32 over a ray query someone else answers, the entries and the radii. A plain
module; everything is seeded, built once per process and never changed."""
import numpy as np

from test_gather import point_mix, unit_vector_model
from test_path_query import probe_case, scene_bounds

f32 = np.float32
OUTPUTS = ("visibility", "bent", "clear", "rays", "rng")
SCENES = ("cornell", "atrium", "tables")  # the Cornell box, the coarse atrium, the tables: sliver-free, so a walk equals the brute force


def closest_hit_occluder(intersect):
    """An any-hit query from a closest-hit one: intersect(org, dirs) -> (t, u, v, tri), a miss at tri = 0xFFFFFFFF; a ray is occluded iff
    its closest hit has t <= tmax (OracleScene.intersect counts hits with t > 1e-4, as the contract does)."""
    def occluded(org, dirs, tmax):
        t, _, _, tri = intersect(org, dirs)
        return (tri != 0xFFFFFFFF) & (t <= tmax)
    return occluded


def oracle_occluder(osc):
    return closest_hit_occluder(lambda o, d: osc.intersect(o, d, False))


def device_occluder(scene):
    """rt_trace_rays RT_QUERY_ANY on the device (Scene.trace): the chain the contract names"""
    return lambda o, d, tmax: scene.trace(o, d, tmax, any_hit=True) == 1


def occlusion_model(occluded, pos, nrm, state, samples, max_dist=None):
    """The contract in numpy fp32 over test_gather.unit_vector_model: per sample the three draws, d = normal + u, l2 = (dx*dx + dy*dy) +
    dz*dz, a DEGENERATE sample where !(l2 > 0) or l2 is not finite, else w = d * (1 / sqrt(l2)) and one any-hit query occluded(org, dirs,
    tmax) -> (m,) bool on the samples that have a direction. max_dist (n,) or None (+inf). -> {"visibility", "bent", "clear", "rays", "rng"}"""
    pos, nrm = np.ascontiguousarray(pos, f32), np.ascontiguousarray(nrm, f32)
    n = len(pos)
    state = np.array(state, np.uint32, copy=True)
    md = np.full(n, np.inf, f32) if max_dist is None else np.ascontiguousarray(max_dist, f32)
    clear, rays, total = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 3), f32)
    for _ in range(samples):
        u, state = unit_vector_model(state)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            d = nrm + u
            l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            ok = (l2 > 0) & np.isfinite(l2)
            w = d * (f32(1.0) / np.sqrt(l2))[:, None]
        assert w.dtype == f32
        at = np.flatnonzero(ok)
        free = np.ones(n, bool)  # a degenerate sample is clear
        if len(at):
            free[at] = ~np.asarray(occluded(pos[at], np.ascontiguousarray(w[at]), md[at]), bool)
        rays += ok.astype(np.uint32)
        clear += free.astype(np.uint32)
        total = np.where((ok & free)[:, None], total + w, total)
    return {"visibility": clear.astype(f32) / f32(samples), "bent": total / f32(samples), "clear": clear, "rays": rays, "rng": state}


RADII = (np.inf, np.inf, 0.25, 0.05, 0.01, -1.0, -0.0, 0.0)  # +inf, the NULL-equivalent, three scene scales, and what occludes nothing


def radius_mix(n, scale, seed):
    """per entry one of +inf (twice: as a value, and as what a NULL max_dist means), 0.25 / 0.05 / 0.01 scene scales, -1, -0.0 and 0;
    +inf and the scales four times as often as each of the last three. (n,) float32"""
    g = np.random.default_rng(seed)
    weight = np.array([4, 4, 4, 4, 4, 1, 1, 1], np.float64)
    kind = g.choice(len(RADII), n, p=weight / weight.sum())
    r = np.array(RADII, f32)
    return np.where((kind >= 2) & (kind <= 4), r[kind] * f32(scale), r[kind]).astype(f32)


HUGE_NORMAL = f32(1e20)  # normal + u overflows l2: every sample of the entry is degenerate


def entries(sd, n, seed):
    """test_gather.point_mix with its special normals, and: entries 4 .. 11 with normals of 1e20 on one to three axes (every sample
    degenerate), entry 12 with the normal exactly the negative of its first unit vector (l2 == 0 on its first sample).
    -> (pos, normal (n, 3) float32, state (n,) uint32, degenerate: the indices of the all-degenerate entries)"""
    pos, nrm, state = point_mix(sd, n, seed)
    degenerate = np.arange(4, min(n, 12))
    for k, i in enumerate(degenerate):
        nrm[i] = np.where((np.arange(3) <= k % 3), HUGE_NORMAL * f32(-1.0 if k & 1 else 1.0), nrm[i])
    if n > 12:
        u, _ = unit_vector_model(state[12:13])
        nrm[12] = -u[0]
        assert (nrm[12] + u[0] == 0).all()
    return pos, nrm, state, degenerate


MIX_N, MIX_SEED, RADIUS_SEED = 1024 + 33, 41, 43  # 17 chunks of 64 entries: one partial; 33 or 34 entries per shard
# the coarse atrium has 235,750 triangles and the expected side is a brute force over them: a prefix of the mix (a mix too), two chunks and one
ENTRIES = {"cornell": MIX_N, "atrium": 129, "tables": MIX_N}
_CASES, _EXPECTED = {}, {}


def mix_case(name):
    """dict(sd, osc, pos, nrm, state, degenerate, radii, scale) of "cornell", "atrium" (coarse) or "tables", built once per process"""
    if name not in _CASES:
        sd, osc, _ = probe_case(name)
        pos, nrm, state, degenerate = entries(sd, MIX_N, MIX_SEED)
        scale = scene_bounds(sd)[2]
        radii = radius_mix(MIX_N, scale, RADIUS_SEED)
        n = ENTRIES[name]
        c = dict(sd=sd, osc=osc, pos=pos[:n].copy(), nrm=nrm[:n].copy(), state=state[:n].copy(), degenerate=degenerate, radii=radii[:n].copy(), scale=scale)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def mix_expected(name, samples, mixed, n=None):
    """occlusion_model over the oracle's brute force on the scene's entries (the first n of them), free or under the radius mix; computed
    once per process and shared read-only"""
    key = (name, samples, mixed, n)
    if key not in _EXPECTED:
        c = mix_case(name)
        out = occlusion_model(oracle_occluder(c["osc"]), c["pos"][:n], c["nrm"][:n], c["state"][:n], samples, c["radii"][:n] if mixed else None)
        for a in out.values():
            a.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


def same(got, want, what, names=OUTPUTS):
    for k in names:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def steps(state, k):
    from test_path_query import xorshift_model
    for _ in range(k):
        _, state = xorshift_model(state)
    return state
