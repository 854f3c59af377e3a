// rt_path_query.hip — path queries: radiance along caller-supplied rays, rt_trace_paths[_device] and their kernel k_path_query.
// (A unit of its own, as rt_query.hip and rt_gbuffer.hip are: a further traversal kernel inside an existing unit changes that unit's
// listings. tests/test_path_query.py runs the ISA hazard scan of tests/test_isa_hazards.py on this unit's listing.)
// The kernel's body is path_rounds (rt_path_rounds.h), shared with k_path_gather; the launch, the checks and the host form's staging are
// rt_query_launch.h's. What is this unit's own: an entry is a ray, org[i] / dir[i], and every path of the entry starts along it.
#include "rt_query_launch.h"
#include "rt_path_rounds.h"

namespace rt {

// k_megakernel's launch shape and round constants (rt_launch.h, rt_kernels.h): the kernel runs the same traversal steps and the same shading
// round under the same register budget
constexpr uint32_t kPathBlock = kMegaBlock, kPathWaves = kMegaWaves;
constexpr int kPathUnroll = 3;          // traversal steps between two checks of the loop's exit condition (kMegaUnroll)
#ifndef RT_PATH_SHADE_PCT
#define RT_PATH_SHADE_PCT 75
#endif
constexpr uint32_t kPathShadePct = RT_PATH_SHADE_PCT; // shade when this share of the live lanes is waiting (kMegaShadePct)
#ifndef RT_PATH_REFILL
#define RT_PATH_REFILL 16
#endif
constexpr uint32_t kPathRefill = RT_PATH_REFILL; // idle lanes after a shading round that make the wave take new rays (kQueryRefill)
static_assert(kPathRefill >= 1u && kPathRefill <= 64u, "a wave has 64 lanes");

// what a launch reads and writes (include/rt_mi355x.h: rt_path_query; NULL outputs are not written)
struct PathDev {
    const float* org;
    const float* dir;
    const uint32_t* rng;
    uint32_t* rng_out;
    float* radiance;
    uint32_t* rays;
    unsigned long long* cursor; // kQueryHeads shard cursors, kQueryHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n, max_depth, samples, rr_start;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

// A path's first ray: get_ray without the camera and without its two draws (rt_device.h: camera_ray's RayData constructor)
RT_DEV RayState path_first_ray(const PathDev& q, uint32_t i, f3 o) {
    RayState r;
    r.org = o;
    r.dir[0] = f2h(q.dir[3 * (size_t)i]), r.dir[1] = f2h(q.dir[3 * (size_t)i + 1]), r.dir[2] = f2h(q.dir[3 * (size_t)i + 2]);
    r.att[0] = r.att[1] = r.att[2] = 0x3C00; // half(1.0)
    r.rad[0] = r.rad[1] = r.rad[2] = 0;      // half(0.0)
    return r;
}

// path_rounds' policy (rt_path_rounds.h): an entry is its origin, inside the contract's range; no draw is taken for a first ray
struct PathRounds {
    static constexpr uint32_t kBlock = kPathBlock, kRefill = kPathRefill, kShadePct = kPathShadePct;
    static constexpr int kUnroll = kPathUnroll;
    RT_DEV static f3 load(const PathDev& q, uint32_t i) { return mk3(q.org[3 * (size_t)i], q.org[3 * (size_t)i + 1], q.org[3 * (size_t)i + 2]); }
    RT_DEV static bool ok(const PathDev& q, f3 o) { return in_contract_range(q.range, o.x, o.y, o.z); }
    RT_DEV static RayState first(const PathDev& q, uint32_t i, f3 o, uint32_t&) { return path_first_ray(q, i, o); }
    RT_DEV static RayState next(const PathDev& q, uint32_t i, uint32_t&) { return path_first_ray(q, i, load(q, i)); } // the same first segment
};

__global__ void __launch_bounds__(kPathBlock, kPathWaves) k_path_query(SceneDev S, PathDev q) { path_rounds<PathRounds>(S, q); }

} // namespace rt

namespace {

PathArgs path_args(const rt_path_query& q) { return {q.n, q.max_depth, q.samples, q.rr_start, q.org, q.dir, q.rng, q.rng_out, q.radiance, q.rays}; }

int path_refuse(const ContractRange& range, const PathArgs& a, uint32_t i) { return refuse_ray_origin(range, a.in0, i); }

int path_enqueue(rt_scene* s, const PathArgs& a, hipStream_t st) {
    PathDev d{};
    d.org = a.in0, d.dir = a.in1, d.rng = a.rng, d.rng_out = a.rng_out, d.radiance = a.radiance, d.rays = a.rays;
    d.n = a.n, d.max_depth = a.max_depth, d.samples = a.samples, d.rr_start = a.rr_start;
    return query_launch(s, kQueryKindPath, k_path_query, kPathBlock, d, a.n, st, s->query_grid[kQueryKindPath] ? nullptr : dev_knob("RT_PATH_GRID"));
}

const PathKind kPathKind = {"org or dir", "ray", path_refuse, path_enqueue};

} // namespace

extern "C" {

int rt_trace_paths(rt_scene* s, const rt_path_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    return paths_host(s, path_args(*q), kPathKind);
}

int rt_trace_paths_device(rt_scene* s, const rt_path_query* q, void* stream) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    return paths_device(s, path_args(*q), kPathKind, (hipStream_t)stream);
}

} // extern "C"
