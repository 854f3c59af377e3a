// rt_occlusion.hip — occlusion gathers: ambient occlusion and the bent normal at caller-supplied points, rt_gather_occlusion[_device], their
// kernel k_occlusion_gather and the C entry of the host diagnostic rt_scene_occlusion_host (the walk itself: scene_check.cpp: occlusion_host).
// (A unit of its own, as rt_query.hip and rt_path_gather.hip are: no existing unit's listing changes. DESIGN.md §26.)
// An occlusion gather is a chain of RT_QUERY_ANY ray queries, as a gather is a chain of path queries: the traversal step is RayFrame<true>'s
// (rt_query.hip) and nothing else — trav_step_wave<false, true>, the lane done at its first counting hit — and no box test, triangle test
// or asm is restated here. The claim of entries is rt_query_frame.h's, the launch and the host form's staging are rt_query_launch.h's.
// What is this unit's own: the FRAME. query_frame<P> retires a lane when its traversal ends; here such a lane books the sample and, while
// the entry has samples left, draws the next direction and starts the next traversal in the same lane. trav_signs is taken once every lane
// of a phase has been started, so a restart belongs between two phases, where the refill stands.
#include "rt_query_launch.h"
#include "rt_query_frame.h"

namespace rt {

constexpr uint32_t kOcclusionBlock = 512; // threads per workgroup: 8 independent waves share one LDS copy of the top of the BVH (as k_query)
constexpr uint32_t kOcclusionWaves = 6;   // waves per SIMD the kernel is compiled for: three workgroups per CU, which is what the LDS allows (as k_query; DESIGN.md §26: 76 VGPRs, none spilled)
#if defined(RT_DEVELOPER_KNOBS) && defined(RT_OCCLUSION_REFILL)
constexpr uint32_t kOcclusionRefill = RT_OCCLUSION_REFILL;
#else
constexpr uint32_t kOcclusionRefill = 16; // lanes of a wave without a running traversal that end its traversal phase (kQueryRefill)
#endif
static_assert(kOcclusionRefill >= 1u && kOcclusionRefill <= 64u, "a wave has 64 lanes");

// what a launch reads and writes (include/rt_mi355x.h: rt_occlusion_query; NULL outputs are not written)
struct OcclusionDev {
    const float* pos;
    const float* normal;
    const float* max_dist;
    const uint32_t* rng;
    uint32_t* rng_out;
    float* visibility;
    float* bent;
    uint32_t* clear;
    uint32_t* rays;
    unsigned long long* cursor; // kQueryHeads shard cursors, kQueryHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n, samples;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

RT_DEV f3 occlusion_load3(const float* p, uint32_t i) { return mk3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }

// What a lane keeps of its entry through the traversal loop: the index, the running state, the samples booked and the rays among them (both
// <= RT_OCCLUSION_MAX_SAMPLES, in one word: booked | rays << 16), the clear count and the running sum. pos, normal and max_dist are re-read
// per sample, as GatherRounds::next re-reads its two; the direction of the sample in flight is the traversal's own T.d.
struct OcclusionLane {
    uint32_t ent, rng, counts, clear;
    f3 sum;
};

// The entry's next samples from the state it holds: DEGENERATE ones are consumed here (three draws each, clear, no ray), a loop bounded by
// `samples`; the first sample with a direction starts its traversal (true). false: the entry has no sample left.
RT_DEV bool occlusion_next(const OcclusionDev& q, OcclusionLane& x, Trav& T, const TravStack& stack) {
    const f3 o = occlusion_load3(q.pos, x.ent), nrm = occlusion_load3(q.normal, x.ent);
    while ((x.counts & 0xFFFFu) < q.samples) {
        const f3 d = nrm + rng_unit_vector(x.rng);
        const float l2 = dot3(d, d);
        if (!(l2 > 0.0f) || !(l2 < __builtin_huge_valf())) { // no direction: no ray, nothing added to the sum
            x.clear++, x.counts++;
            continue;
        }
        const float inv = inv_sqrt2(l2);
        trav_begin(T, o, mk3(d.x * inv, d.y * inv, d.z * inv), stack);
        T.best.t = q.max_dist ? q.max_dist[x.ent] : __builtin_huge_valf();
        return true;
    }
    return false;
}

// the sample whose traversal has ended: T.d is its direction, a hit in T.best says occluded
RT_DEV void occlusion_book(OcclusionLane& x, const Trav& T) {
    x.counts += 0x10001u; // one sample, one ray
    if (T.best.tri == kNoTri) x.clear++, x.sum = x.sum + T.d;
}

RT_DEV void occlusion_store(const OcclusionDev& q, const OcclusionLane& x) {
    const float n = (float)q.samples;
    const size_t i = x.ent;
    if (q.visibility) q.visibility[i] = (float)x.clear / n;
    if (q.bent) q.bent[3 * i] = x.sum.x / n, q.bent[3 * i + 1] = x.sum.y / n, q.bent[3 * i + 2] = x.sum.z / n;
    if (q.clear) q.clear[i] = x.clear;
    if (q.rays) q.rays[i] = x.counts >> 16;
    if (q.rng_out) q.rng_out[i] = x.rng;
}

// entry i into the calling lane: true, its first traversal runs; false, it was rejected (marked, no draw taken) or every sample of it was
// degenerate (stored), and the lane takes the next entry
RT_DEV bool occlusion_start(const OcclusionDev& q, uint32_t i, OcclusionLane& x, Trav& T, const TravStack& stack) {
    const f3 o = occlusion_load3(q.pos, i), nrm = occlusion_load3(q.normal, i);
    const float md = q.max_dist ? q.max_dist[i] : __builtin_huge_valf();
    const uint32_t a = q.rng[i];
    if (!(in_contract_range(q.range, o.x, o.y, o.z) && __builtin_isfinite(nrm.x) && __builtin_isfinite(nrm.y) && __builtin_isfinite(nrm.z) && md == md)) {
        const float nan = __builtin_nanf("");
        if (q.visibility) q.visibility[i] = nan;
        if (q.bent) q.bent[3 * (size_t)i] = nan, q.bent[3 * (size_t)i + 1] = nan, q.bent[3 * (size_t)i + 2] = nan;
        if (q.clear) q.clear[i] = 0xFFFFFFFFu;
        if (q.rays) q.rays[i] = 0xFFFFFFFFu;
        if (q.rng_out) q.rng_out[i] = a;
        return false;
    }
    x.ent = i, x.rng = a, x.counts = 0u, x.clear = 0u, x.sum = mk3(0.0f, 0.0f, 0.0f);
    if (occlusion_next(q, x, T, stack)) return true;
    occlusion_store(q, x);
    return false;
}

// The frame. Persistent waves, one lane per entry. A round: the traversal phase has ended; the lanes whose traversal is complete book
// their sample; those with samples left restart, those with none store their entry and fall free; the free lanes are refilled from the
// shard cursors; the next phase runs until kOcclusionRefill lanes have no running traversal (all 64 once every shard is exhausted). The
// wave ends when every shard is exhausted and no lane is busy: a lane that is done traversing but has samples left is busy, so the test is
// on `busy`, not on T.cur. No lane waits for another wave; the only barrier is the LDS fill's, before the loop.
__global__ void __launch_bounds__(kOcclusionBlock, kOcclusionWaves) k_occlusion_gather(SceneDev S, OcclusionDev q) {
    RT_TRAVERSAL_LDS(kOcclusionBlock)
    Trav T;
    T.cur = kTravDone;
    OcclusionLane x{};
    bool busy = false;
    Claim claim = claim_begin();
    for (;;) {
        if (busy && T.cur == kTravDone) {
            occlusion_book(x, T);
            busy = occlusion_next(q, x, T, stack);
            if (!busy) occlusion_store(q, x);
        }
        claim = claim_refill(claim, ClaimList{q.cursor, q.n}, [&] { return !busy; }, [&](uint32_t i) { busy = occlusion_start(q, i, x, T, stack); });
        if (__ballot(busy) == 0ull) break; // (a lane is free after the refill only when every shard is exhausted)
        const TravSigns sg = trav_signs(T); // every ray of this phase has been started by now
        const uint32_t stop = claim_exhausted(claim) ? 64u : kOcclusionRefill;
        while (count(trav_done(T)) < stop) {
            (void)trav_step_wave<false, true>(S, T, stack, top, sg);
            if (T.best.tri != kNoTri) T.cur = kTravDone; // ANY: done at the first counting hit (RayFrame<true>::step)
        }
    }
}

} // namespace rt

namespace {

// the refusals, in rt_trace_rays' order (rt_query.hip: query_check)
int occlusion_check(const rt_scene* s, const rt_occlusion_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->n == 0) return RT_OK;
    if (q->samples < 1 || q->samples > RT_OCCLUSION_MAX_SAMPLES) return fail(RT_ERR_INVALID, "samples must be 1 .. " + std::to_string(RT_OCCLUSION_MAX_SAMPLES));
    if (!q->pos || !q->normal) return fail(RT_ERR_INVALID, "null pos or normal");
    if (!q->rng) return fail(RT_ERR_INVALID, "null rng: every entry needs its xorshift32 state");
    if (!q->visibility && !q->bent && !q->clear && !q->rays) return fail(RT_ERR_INVALID, "occlusion gather with every output NULL");
    return refuse_host_only(s);
}

// fills the launch struct and hands it to the shared launch (PRE: occlusion_check passed, n > 0, pointers on the scene's device)
int occlusion_enqueue(rt_scene* s, const rt_occlusion_query* q, hipStream_t st) {
    OcclusionDev d{};
    d.pos = q->pos, d.normal = q->normal, d.max_dist = q->max_dist, d.rng = q->rng, d.rng_out = q->rng_out;
    d.visibility = q->visibility, d.bent = q->bent, d.clear = q->clear, d.rays = q->rays;
    d.n = q->n, d.samples = q->samples;
    return query_launch(s, kQueryKindOcclusion, k_occlusion_gather, kOcclusionBlock, d, q->n, st,
                        s->query_grid[kQueryKindOcclusion] ? nullptr : dev_knob("RT_OCCLUSION_GRID"));
}

} // namespace

extern "C" {

int rt_gather_occlusion(rt_scene* s, const rt_occlusion_query* q) {
    if (const int rc = occlusion_check(s, q)) return rc;
    const uint32_t n = q->n;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < n; ++i) {
        const float* o = q->pos + 3 * (size_t)i;
        const float* v = q->normal + 3 * (size_t)i;
        if (!in_contract_range(range, o[0], o[1], o[2]))
            return fail(RT_ERR_INVALID, "entry " + std::to_string(i) + ": position more than 100 scene scales outside the scene's bounds or not finite (outside the range of the closest-hit contract)");
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return fail(RT_ERR_INVALID, "entry " + std::to_string(i) + ": normal not finite");
        if (q->max_dist && std::isnan(q->max_dist[i])) return fail(RT_ERR_INVALID, "entry " + std::to_string(i) + ": max_dist is NaN");
    }
    const StageIn ins[4] = {{q->pos, 12}, {q->normal, 12}, {q->max_dist, 4}, {q->rng, 4}};
    const StageOut outs[5] = {{q->visibility, 4}, {q->bent, 12}, {q->clear, 4}, {q->rays, 4}, {q->rng_out, 4, 3}}; // rng_out: in place on the device, in rng's buffer
    return query_staged(s, n, ins, outs, [&](void* const* in, void* const* out) {
        rt_occlusion_query d{};
        d.n = n, d.samples = q->samples;
        d.pos = (const float*)in[0], d.normal = (const float*)in[1], d.max_dist = (const float*)in[2], d.rng = (const uint32_t*)in[3];
        d.visibility = (float*)out[0], d.bent = (float*)out[1], d.clear = (uint32_t*)out[2], d.rays = (uint32_t*)out[3], d.rng_out = (uint32_t*)out[4];
        return occlusion_enqueue(s, &d, 0);
    });
}

int rt_gather_occlusion_device(rt_scene* s, const rt_occlusion_query* q, void* stream) {
    if (const int rc = occlusion_check(s, q)) return rc;
    if (q->n == 0) return RT_OK;
    return occlusion_enqueue(s, q, (hipStream_t)stream);
}

int rt_scene_occlusion_host(const rt_scene* s, const rt_occlusion_query* q, int use_bvh, uint64_t* node_visits, uint64_t* tri_tests) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->n && (!q->pos || !q->normal || !q->rng)) return fail(RT_ERR_INVALID, "null pos, normal or rng");
    if (const int rc0 = sync_host_copy(s)) return rc0;
    std::string err;
    const int rc = no_throw([&] {
        return occlusion_host(s->hs, q->n, q->samples, q->pos, q->normal, q->max_dist, q->rng, use_bvh, q->rng_out, q->visibility, q->bent, q->clear,
                              q->rays, node_visits, tri_tests, err);
    });
    return rc == RT_OK ? RT_OK : fail(rc, err.empty() ? g_err : err);
}

} // extern "C"
