// rt_path_gather.hip — gather queries: diffuse-lobe radiance at caller-supplied points, rt_gather_paths[_device] and their kernel k_path_gather.
// (A unit of its own, as rt_path_query.hip is: a further traversal kernel inside an existing unit changes that unit's listings.
// tests/test_gather.py runs the ISA hazard scan of tests/test_isa_hazards.py on this unit's listing.)
// The kernel's body is path_rounds (rt_path_rounds.h), shared with k_path_query; the launch, the checks and the host form's staging are
// rt_query_launch.h's. What is this unit's own: an entry is a point and a normal, pos[i] / normal[i], an entry with a non-finite normal is
// rejected too, and every path of the entry starts along a direction of its own, three draws on the entry's running state.
#include "rt_query_launch.h"
#include "rt_path_rounds.h"

namespace rt {

// k_path_query's launch shape and round constants (rt_path_query.hip)
constexpr uint32_t kGatherBlock = kMegaBlock, kGatherWaves = kMegaWaves;
constexpr int kGatherUnroll = 3;          // traversal steps between two checks of the loop's exit condition (kMegaUnroll)
#ifndef RT_GATHER_SHADE_PCT
#define RT_GATHER_SHADE_PCT 75
#endif
constexpr uint32_t kGatherShadePct = RT_GATHER_SHADE_PCT; // shade when this share of the live lanes is waiting (kMegaShadePct)
#ifndef RT_GATHER_REFILL
#define RT_GATHER_REFILL 16
#endif
constexpr uint32_t kGatherRefill = RT_GATHER_REFILL; // idle lanes after a shading round that make the wave take new entries (kQueryRefill)
static_assert(kGatherRefill >= 1u && kGatherRefill <= 64u, "a wave has 64 lanes");

// what a launch reads and writes (include/rt_mi355x.h: rt_gather_query; NULL outputs are not written)
struct GatherDev {
    const float* pos;
    const float* normal;
    const uint32_t* rng;
    uint32_t* rng_out;
    float* radiance;
    uint32_t* rays;
    unsigned long long* cursor; // kQueryHeads shard cursors, kQueryHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n, max_depth, samples, rr_start;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

RT_DEV f3 gather_load3(const float* p, uint32_t i) { return mk3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }

// A path's first ray: the diffuse bounce's own scattered ray (rt_device.h: scatter, normal + rng_unit_vector, without the near_zero clause,
// which tests an incoming direction that does not exist here) from pos[i], with the attenuation and radiance of a camera ray. Three draws.
RT_DEV RayState gather_first_ray(uint32_t& rng, f3 o, f3 nrm) {
    RayState r;
    const f3 d = nrm + rng_unit_vector(rng);
    r.org = o;
    r.dir[0] = f2h(d.x), r.dir[1] = f2h(d.y), r.dir[2] = f2h(d.z);
    r.att[0] = r.att[1] = r.att[2] = 0x3C00; // half(1.0)
    r.rad[0] = r.rad[1] = r.rad[2] = 0;      // half(0.0)
    return r;
}

// path_rounds' policy (rt_path_rounds.h): an entry is a position and a normal, both finite; every path draws its own first direction
struct GatherEntry { f3 o, nrm; };
struct GatherRounds {
    static constexpr uint32_t kBlock = kGatherBlock, kRefill = kGatherRefill, kShadePct = kGatherShadePct;
    static constexpr int kUnroll = kGatherUnroll;
    RT_DEV static GatherEntry load(const GatherDev& q, uint32_t i) { return {gather_load3(q.pos, i), gather_load3(q.normal, i)}; }
    RT_DEV static bool ok(const GatherDev& q, const GatherEntry& e) {
        return in_contract_range(q.range, e.o.x, e.o.y, e.o.z) && __builtin_isfinite(e.nrm.x) && __builtin_isfinite(e.nrm.y) && __builtin_isfinite(e.nrm.z);
    }
    RT_DEV static RayState first(const GatherDev&, uint32_t, const GatherEntry& e, uint32_t& a) { return gather_first_ray(a, e.o, e.nrm); }
    RT_DEV static RayState next(const GatherDev& q, uint32_t i, uint32_t& rng) { return gather_first_ray(rng, gather_load3(q.pos, i), gather_load3(q.normal, i)); }
};

__global__ void __launch_bounds__(kGatherBlock, kGatherWaves) k_path_gather(SceneDev S, GatherDev q) { path_rounds<GatherRounds>(S, q); }

} // namespace rt

namespace {

PathArgs gather_args(const rt_gather_query& q) { return {q.n, q.max_depth, q.samples, q.rr_start, q.pos, q.normal, q.rng, q.rng_out, q.radiance, q.rays}; }

int gather_refuse(const ContractRange& range, const PathArgs& a, uint32_t i) {
    const float* o = a.in0 + 3 * (size_t)i;
    const float* v = a.in1 + 3 * (size_t)i;
    if (!in_contract_range(range, o[0], o[1], o[2]))
        return fail(RT_ERR_INVALID, "entry " + std::to_string(i) + ": position more than 100 scene scales outside the scene's bounds or not finite (outside the range of the closest-hit contract)");
    if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return fail(RT_ERR_INVALID, "entry " + std::to_string(i) + ": normal not finite");
    return RT_OK;
}

int gather_enqueue(rt_scene* s, const PathArgs& a, hipStream_t st) {
    GatherDev d{};
    d.pos = a.in0, d.normal = a.in1, d.rng = a.rng, d.rng_out = a.rng_out, d.radiance = a.radiance, d.rays = a.rays;
    d.n = a.n, d.max_depth = a.max_depth, d.samples = a.samples, d.rr_start = a.rr_start;
    return query_launch(s, kQueryKindGather, k_path_gather, kGatherBlock, d, a.n, st, s->query_grid[kQueryKindGather] ? nullptr : dev_knob("RT_GATHER_GRID"));
}

const PathKind kGatherKind = {"pos or normal", "entry", gather_refuse, gather_enqueue};

} // namespace

extern "C" {

int rt_gather_paths(rt_scene* s, const rt_gather_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    return paths_host(s, gather_args(*q), kGatherKind);
}

int rt_gather_paths_device(rt_scene* s, const rt_gather_query* q, void* stream) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    return paths_device(s, gather_args(*q), kGatherKind, (hipStream_t)stream);
}

} // extern "C"
