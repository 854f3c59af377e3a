// rt_query.hip — ray queries with a per-ray tmax: rt_trace_rays[_device] (closest hit, occlusion) and their kernel k_query<ANY>.
// (A unit of its own, as rt_gbuffer.hip is: a second traversal kernel beside k_intersect_batch in rt_probes.hip changes that kernel's
// listing. tests/test_ray_query.py runs the ISA hazard scan of tests/test_isa_hazards.py on this unit's listing.)
// The kernel's body is query_frame (rt_query_frame.h), shared with k_closest, with the claim every query kernel shares; the launch and the host
// form's staging are rt_query_launch.h's. What is this unit's own: an entry is a ray with a tmax, and a step is the ray traversal's.
#include "rt_query_launch.h"
#include "rt_query_frame.h"

namespace rt {

constexpr uint32_t kQueryBlock = 512; // threads per workgroup: 8 independent waves share one LDS copy of the top of the BVH (as k_megakernel)
constexpr uint32_t kQueryWaves = 6;   // waves per SIMD the kernel is compiled for (k_megakernel's budget: 80 VGPRs)
constexpr uint32_t kQueryRefill = 16; // idle lanes of a wave that end its traversal phase: they write their results and take new rays
// (the shards, their cursors and the claim size — kQueryHeads, kQueryHeadStride, kQueryChunk — are rt_internal.h's, shared with the other query kinds)

// what a launch reads and writes (include/rt_mi355x.h: rt_ray_query; NULL outputs are not written)
struct QueryDev {
    const float* org;
    const float* dir;
    const float* tmax;
    float* t;
    float* u;
    float* v;
    uint32_t* tri;
    uint8_t* occluded;
    unsigned long long* cursor; // kQueryHeads shard cursors, kQueryHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

// query_frame's policy (rt_query_frame.h): an entry is a ray and its tmax, the origin inside the contract's range and tmax no NaN; a step
// is the ray traversal's whole-leaf step (trav_step_wave<false, true>).
// tmax: the closest hit starts at best.t = tmax, tri = kNoTri. The box test culls against best.t and keeps boxes at equal distance,
// tri_test_regs takes t < best.t or t == best.t at a lower index: a hit counts iff kTNear < t <= tmax, and the closest counting hit is the
// closest hit when that is <= tmax. ANY: a lane ends at its first counting hit.
template <bool ANY>
struct RayFrame {
    static constexpr uint32_t kBlock = kQueryBlock, kRefill = kQueryRefill;
    struct Lane {};
    RT_DEV static bool start(const QueryDev& q, uint32_t i, Trav& T, const TravStack& stack) {
        const size_t k = 3 * (size_t)i;
        const f3 o = mk3(q.org[k], q.org[k + 1], q.org[k + 2]);
        const f3 d = mk3(q.dir[k], q.dir[k + 1], q.dir[k + 2]);
        const float tm = q.tmax ? q.tmax[i] : __builtin_huge_valf();
        if (in_contract_range(q.range, o.x, o.y, o.z) && tm == tm) {
            trav_begin(T, o, d, stack);
            T.best.t = tm;
            return true;
        }
        if (ANY) { // rejected: marked, never traced
            q.occluded[i] = 2u;
        } else {
            if (q.t) q.t[i] = __builtin_nanf("");
            if (q.tri) q.tri[i] = RT_TRI_REJECTED;
        }
        return false;
    }
    RT_DEV static TravSigns phase(const Trav& T) { return trav_signs(T); }
    RT_DEV static void step(const SceneDev& S, Trav& T, Lane&, const TravStack& stack, const TopTree& top, const TravSigns& sg) {
        (void)trav_step_wave<false, true>(S, T, stack, top, sg);
        if (ANY && T.best.tri != kNoTri) T.cur = kTravDone;
    }
    RT_DEV static void store(const QueryDev& q, uint32_t i, const Trav& T, const Lane&) {
        const bool hit = T.best.tri != kNoTri;
        if (ANY) {
            q.occluded[i] = hit ? 1u : 0u;
        } else {
            if (q.t) q.t[i] = hit ? T.best.t : __builtin_huge_valf(); // a miss: best.t still holds tmax
            if (q.u) q.u[i] = T.best.u;
            if (q.v) q.v[i] = T.best.v;
            if (q.tri) q.tri[i] = T.best.tri;
        }
    }
};

template <bool ANY>
__global__ void __launch_bounds__(kQueryBlock, kQueryWaves) k_query(SceneDev S, QueryDev q) { query_frame<RayFrame<ANY>>(S, q); }

} // namespace rt

namespace {

int query_check(const rt_scene* s, const rt_ray_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->mode != RT_QUERY_CLOSEST && q->mode != RT_QUERY_ANY) return fail(RT_ERR_INVALID, "unknown query mode");
    if (q->n == 0) return RT_OK;
    if (!q->org || !q->dir) return fail(RT_ERR_INVALID, "null org or dir");
    if (q->mode == RT_QUERY_ANY && !q->occluded) return fail(RT_ERR_INVALID, "RT_QUERY_ANY needs the occluded output");
    if (q->mode == RT_QUERY_CLOSEST && !q->t && !q->u && !q->v && !q->tri) return fail(RT_ERR_INVALID, "RT_QUERY_CLOSEST with every output NULL");
    return refuse_host_only(s);
}

// fills the launch struct and hands it to the shared launch (PRE: query_check passed, n > 0, pointers on the scene's device)
int query_enqueue(rt_scene* s, const rt_ray_query* q, hipStream_t st) {
    const bool any = q->mode == RT_QUERY_ANY;
    QueryDev d{};
    d.org = q->org, d.dir = q->dir, d.tmax = q->tmax;
    d.t = any ? nullptr : q->t, d.u = any ? nullptr : q->u, d.v = any ? nullptr : q->v, d.tri = any ? nullptr : q->tri;
    d.occluded = any ? q->occluded : nullptr;
    d.n = q->n;
    const QueryKind kind = any ? kQueryKindAny : kQueryKindClosest;
    return query_launch(s, kind, any ? k_query<true> : k_query<false>, kQueryBlock, d, q->n, st, s->query_grid[kind] ? nullptr : dev_knob("RT_QUERY_GRID"));
}

} // namespace

extern "C" {

int rt_trace_rays(rt_scene* s, const rt_ray_query* q) {
    if (const int rc = query_check(s, q)) return rc;
    const uint32_t n = q->n;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < n; ++i) {
        if (const int rc = refuse_ray_origin(range, q->org, i)) return rc;
        if (q->tmax && std::isnan(q->tmax[i])) return fail(RT_ERR_INVALID, "ray " + std::to_string(i) + ": tmax is NaN");
    }
    const bool any = q->mode == RT_QUERY_ANY;
    const StageIn ins[3] = {{q->org, 12}, {q->dir, 12}, {q->tmax, 4}};
    const StageOut outs[5] = {{any ? nullptr : q->t, 4}, {any ? nullptr : q->u, 4}, {any ? nullptr : q->v, 4}, {any ? nullptr : q->tri, 4}, {any ? q->occluded : nullptr, 1}};
    return query_staged(s, n, ins, outs, [&](void* const* in, void* const* out) {
        rt_ray_query d{};
        d.n = n, d.mode = q->mode;
        d.org = (const float*)in[0], d.dir = (const float*)in[1], d.tmax = (const float*)in[2];
        d.t = (float*)out[0], d.u = (float*)out[1], d.v = (float*)out[2], d.tri = (uint32_t*)out[3], d.occluded = (uint8_t*)out[4];
        return query_enqueue(s, &d, 0);
    });
}

int rt_trace_rays_device(rt_scene* s, const rt_ray_query* q, void* stream) {
    if (const int rc = query_check(s, q)) return rc;
    if (q->n == 0) return RT_OK;
    return query_enqueue(s, q, (hipStream_t)stream);
}

} // extern "C"
