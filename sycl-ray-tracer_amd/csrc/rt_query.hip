// rt_query.hip — ray queries with a per-ray tmax: rt_trace_rays[_device] (closest hit, occlusion) and their kernel k_query<ANY>.
// (A unit of its own, as rt_gbuffer.hip is: a second traversal kernel beside k_intersect_batch in rt_probes.hip changes that kernel's
// listing. tests/test_ray_query.py runs the ISA hazard scan of tests/test_isa_hazards.py on this unit's listing.)
#include "rt_query_launch.h"
#include "rt_device.h"

namespace rt {

constexpr uint32_t kQueryBlock = 512; // threads per workgroup: 8 independent waves share one LDS copy of the top of the BVH (as k_megakernel)
constexpr uint32_t kQueryWaves = 6;   // waves per SIMD the kernel is compiled for (k_megakernel's budget: 80 VGPRs)
constexpr uint32_t kQueryRefill = 16; // idle lanes of a wave that end its traversal phase: they write their results and take new rays
// (the shards, their cursors and the claim size — kQueryHeads, kQueryHeadStride, kQueryChunk — are rt_internal.h's, shared with the path and gather queries)

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
    unsigned long long n;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

RT_DEV unsigned long long uniform64(unsigned long long x) {
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}

// Persistent waves. A wave claims kQueryChunk rays at a time from a shard cursor (above) and hands them to its idle lanes, traverses whole-leaf
// steps (trav_step_wave<false, true>) until kQueryRefill of its lanes are idle, writes their results and refills them: a lane whose ray was
// short takes the next one instead of waiting for the wave's longest (rt_intersect_batch's kernel runs each wave until its slowest lane is
// done). Once every shard is exhausted the wave traverses until all its lanes are done and ends. No wave waits for another: the barrier of
// RT_TRAVERSAL_LDS (the staged top of the tree) comes before the loop, and every loop ends when the shards are exhausted.
// tmax: the closest hit starts at best.t = tmax, tri = kNoTri. The box test culls against best.t and keeps boxes at equal distance,
// tri_test_regs takes t < best.t or t == best.t at a lower index: a hit counts iff kTNear < t <= tmax, and the closest counting hit is the
// closest hit when that is <= tmax. ANY: a lane ends at its first counting hit.
template <bool ANY>
__global__ void __launch_bounds__(kQueryBlock, kQueryWaves) k_query(SceneDev S, QueryDev q) {
    RT_TRAVERSAL_LDS(kQueryBlock)
    Trav T;
    T.cur = kTravDone;
    unsigned long long ray = 0; // the lane's ray while `busy`
    bool busy = false;
    // wave-uniform: the shard drawn on, shards found exhausted, the claimed rays not yet handed out [cb, ce)
    uint32_t head = blockIdx.x % kQueryHeads, heads_done = 0;
    unsigned long long cb = 0, ce = 0;
    for (;;) {
        // REFILL every idle lane (or until every shard is exhausted)
        for (;;) {
            const lmask idle = __ballot(!busy);
            const uint32_t cnt = (uint32_t)__popcll(idle);
            if (cnt == 0u) break;
            while (cb == ce && heads_done < kQueryHeads) { // claim: the next chunk of this shard, or move on to the next shard
                const unsigned long long lo = q.n * head / kQueryHeads, len = q.n * (head + 1u) / kQueryHeads - lo;
                unsigned long long o = 0;
                if ((threadIdx.x & 63u) == 0u) o = atomicAdd(q.cursor + head * kQueryHeadStride, (unsigned long long)kQueryChunk);
                o = uniform64(o);
                if (o < len) {
                    cb = lo + o, ce = lo + (o + kQueryChunk < len ? o + kQueryChunk : len);
                } else {
                    head = head + 1u == kQueryHeads ? 0u : head + 1u, heads_done++;
                }
            }
            if (cb == ce) break; // every shard exhausted
            const uint32_t take = ce - cb < cnt ? (uint32_t)(ce - cb) : cnt;
            const uint32_t rank = lane_rank(idle);
            if (!busy && rank < take) {
                const unsigned long long i = cb + rank;
                const f3 o = mk3(q.org[3 * i], q.org[3 * i + 1], q.org[3 * i + 2]);
                const f3 d = mk3(q.dir[3 * i], q.dir[3 * i + 1], q.dir[3 * i + 2]);
                const float tm = q.tmax ? q.tmax[i] : __builtin_huge_valf();
                if (in_contract_range(q.range, o.x, o.y, o.z) && tm == tm) {
                    trav_begin(T, o, d, stack);
                    T.best.t = tm;
                    ray = i, busy = true;
                } else if (ANY) { // rejected: marked, never traced (the lane stays idle and takes the next ray)
                    q.occluded[i] = 2u;
                } else {
                    if (q.t) q.t[i] = __builtin_nanf("");
                    if (q.tri) q.tri[i] = RT_TRI_REJECTED;
                }
            }
            cb += take;
        }
        const bool exhausted = cb == ce && heads_done == kQueryHeads;
        if (__ballot(busy) == 0ull) break; // (a lane is idle after the refill only when every shard is exhausted)
        const TravSigns sg = trav_signs(T); // every ray of this phase has been started
        const uint32_t stop = exhausted ? 64u : kQueryRefill;
        while ((uint32_t)__popcll(__ballot(T.cur == kTravDone)) < stop) {
            (void)trav_step_wave<false, true>(S, T, stack, top, sg);
            if (ANY && T.best.tri != kNoTri) T.cur = kTravDone;
        }
        if (busy && T.cur == kTravDone) {
            const bool hit = T.best.tri != kNoTri;
            if (ANY) {
                q.occluded[ray] = hit ? 1u : 0u;
            } else {
                if (q.t) q.t[ray] = hit ? T.best.t : __builtin_huge_valf(); // a miss: best.t still holds tmax
                if (q.u) q.u[ray] = T.best.u;
                if (q.v) q.v[ray] = T.best.v;
                if (q.tri) q.tri[ray] = T.best.tri;
            }
            busy = false;
        }
    }
}

} // namespace rt

namespace {

int query_check(const rt_scene* s, const rt_ray_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->mode != RT_QUERY_CLOSEST && q->mode != RT_QUERY_ANY) return fail(RT_ERR_INVALID, "unknown query mode");
    if (q->n == 0) return RT_OK;
    if (!q->org || !q->dir) return fail(RT_ERR_INVALID, "null org or dir");
    if (q->mode == RT_QUERY_ANY && !q->occluded) return fail(RT_ERR_INVALID, "RT_QUERY_ANY needs the occluded output");
    if (q->mode == RT_QUERY_CLOSEST && !q->t && !q->u && !q->v && !q->tri) return fail(RT_ERR_INVALID, "RT_QUERY_CLOSEST with every output NULL");
    if (s->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    return RT_OK;
}

// fills the launch struct and hands it to the shared launch (PRE: query_check passed, n > 0, pointers on the scene's device)
int query_enqueue(rt_scene* s, const rt_ray_query* q, hipStream_t st) {
    const bool any = q->mode == RT_QUERY_ANY;
    QueryDev d{};
    d.org = q->org, d.dir = q->dir, d.tmax = q->tmax;
    d.t = any ? nullptr : q->t, d.u = any ? nullptr : q->u, d.v = any ? nullptr : q->v, d.tri = any ? nullptr : q->tri;
    d.occluded = any ? q->occluded : nullptr;
    d.n = q->n;
    if (any) return query_launch(s, kQueryKindAny, k_query<true>, kQueryBlock, d, q->n, st);
    return query_launch(s, kQueryKindClosest, k_query<false>, kQueryBlock, d, q->n, st);
}

} // namespace

extern "C" {

int rt_trace_rays(rt_scene* s, const rt_ray_query* q) {
    if (const int rc = query_check(s, q)) return rc;
    const uint32_t n = q->n;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < n; ++i) {
        const float* o = q->org + 3 * (size_t)i;
        if (!in_contract_range(range, o[0], o[1], o[2]))
            return fail(RT_ERR_INVALID, "ray " + std::to_string(i) + ": origin more than 100 scene scales outside the scene's bounds or not finite (outside the range of the closest-hit contract)");
        if (q->tmax && std::isnan(q->tmax[i])) return fail(RT_ERR_INVALID, "ray " + std::to_string(i) + ": tmax is NaN");
    }
    HIPCHK(hipSetDevice(s->device));
    const bool any = q->mode == RT_QUERY_ANY;
    DevBuf b_org, b_dir, b_tmax, b_t, b_u, b_v, b_tri, b_occ;
    HIPCHK(b_org.alloc((size_t)n * 12));
    HIPCHK(b_dir.alloc((size_t)n * 12));
    HIPCHK(hipMemcpy(b_org.p, q->org, (size_t)n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_dir.p, q->dir, (size_t)n * 12, hipMemcpyHostToDevice));
    rt_ray_query d{};
    d.n = n, d.mode = q->mode;
    d.org = b_org.as<float>(), d.dir = b_dir.as<float>();
    if (q->tmax) {
        HIPCHK(b_tmax.alloc((size_t)n * 4));
        HIPCHK(hipMemcpy(b_tmax.p, q->tmax, (size_t)n * 4, hipMemcpyHostToDevice));
        d.tmax = b_tmax.as<float>();
    }
    struct Out { void* host; DevBuf* buf; size_t bytes; };
    const Out outs[5] = {{any ? nullptr : q->t, &b_t, 4}, {any ? nullptr : q->u, &b_u, 4}, {any ? nullptr : q->v, &b_v, 4},
                         {any ? nullptr : q->tri, &b_tri, 4}, {any ? q->occluded : nullptr, &b_occ, 1}};
    for (const Out& o : outs)
        if (o.host) HIPCHK(o.buf->alloc((size_t)n * o.bytes));
    d.t = b_t.as<float>(), d.u = b_u.as<float>(), d.v = b_v.as<float>(), d.tri = b_tri.as<uint32_t>(), d.occluded = b_occ.as<uint8_t>();
    if (const int rc = query_enqueue(s, &d, 0)) return rc;
    HIPCHK(hipStreamSynchronize(0));
    for (const Out& o : outs)
        if (o.host) HIPCHK(hipMemcpy(o.host, o.buf->p, (size_t)n * o.bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_trace_rays_device(rt_scene* s, const rt_ray_query* q, void* stream) {
    if (const int rc = query_check(s, q)) return rc;
    if (q->n == 0) return RT_OK;
    return query_enqueue(s, q, (hipStream_t)stream);
}

} // extern "C"
