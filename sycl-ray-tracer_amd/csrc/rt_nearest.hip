// rt_nearest.hip — k-nearest closest-point queries: rt_closest_points_multi[_device], the k nearest counting triangles of every point in
// (dist2, index) order, resumable with a key; their kernel k_nearest<N> and the C entry of the host diagnostic rt_scene_nearest_host (the
// walk itself: scene_check.cpp: nearest_host).
// (A unit of its own, as rt_closest.hip and rt_multihit.hip are: no other unit's listing changes. DESIGN.md §25.)
// The kernel's body is query_frame (rt_query_frame.h) with the claim every query kernel shares; the launch and the host form's staging are
// rt_query_launch.h's. No arithmetic is restated here: the candidate and the winner rule are rt_closest_point.h's, the start of a
// traversal and the inner step are rt_closest_step.h's (k_closest's own), the list — its state, opening, key-and-duplicate test,
// insertion and store — is rt_hit_list.h's, the whole-leaf read is rt_whole_leaf.h's. What is this unit's own: an entry is a point with
// a max_dist2 and a key, T.best is not the answer but the BOUND, and the candidate that the leaf step hands the list.
// What it relies on in rt_closest_step.h and the trees (held by tests/test_nearest.py: test_what_the_kernel_relies_on_in_the_point_traversal):
// cur == 0 only in a point's first step (closest_begin alone sets it, no node has the root as a child), and closest_inner reads nothing of
// T.best but best.t — so k and the key can travel in best.u / v / tri to that first step.
#include "rt_query_launch.h"
#include "rt_query_frame.h"
#include "rt_closest_point.h"
#include "rt_closest_step.h"
#include "rt_hit_list.h"
#include "rt_whole_leaf.h"

namespace rt {

constexpr uint32_t kNearestBlock = 512; // threads per workgroup: 8 independent waves share one LDS copy of the top of the BVH (as k_closest)
constexpr uint32_t kNearestRefill = 16; // idle lanes of a wave that end its traversal phase: they write their results and take new points
// waves per SIMD an instantiation is compiled for, the most at which it spills no VGPR (a workgroup is two waves per SIMD, so 2, 4 or 6):
// a list of N slots is 4 N registers beside the point traversal's 56. Two and four slots fit k_closest's budget (6 waves, 80 VGPRs: 74 and
// 79 used); eight at 6 waves spill, so that list is compiled for 4 waves (two workgroups per CU: 112 VGPRs, none spilled). DESIGN.md §25:
// the resources per instantiation.
template <uint32_t N> constexpr uint32_t kNearestWaves = N > 4 ? 4 : 6;

// what a launch reads and writes (include/rt_mi355x.h: rt_nearest_query; NULL outputs are not written)
struct NearestDev {
    const float* pos;
    const float* max_dist2;
    const float* after_dist2;
    const uint32_t* after_tri;
    float* dist2;
    float* u;
    float* v;
    uint32_t* tri;
    uint32_t* count;
    unsigned long long* cursor; // kQueryHeads shard cursors, kQueryHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n, k;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

// THE LIST is rt_hit_list.h's with Hit::t = dist2: slot N - 1 IS T.best, the bound closest_inner culls against. A free slot holds
// (max_dist2, 0, 0, kNoTri): every counting candidate sorts before it (dist2 <= max_dist2, index < kNoTri), so filling the list and
// replacing its last entry are one insertion, and the bound is (max_dist2, kNoTri) while a slot is free and (dist2, tri) of the k-th entry
// once none is — by closest_better, dist2 < best or dist2 == best at a lower index, a candidate passes exactly when it counts against
// max_dist2 and sorts before the k-th entry. closest_inner enters a child at lb * kClosestSlack <= best.t: a candidate that ties with
// the k-th entry at a lower index is still reached, and §22's cull argument — about the candidate's underestimate of the true distance,
// whatever the bound is — holds for a bound that only ever moves down. The key (HitList's after_t holds after_dist2) filters candidates
// and culls no box.

// One candidate: the contract's text on the record's ten live dwords, the winner rule against the bound (a NaN dist2 fails it; so does
// the bound's own triangle met again: it ties with itself), the key and the de-duplication against the other slots (hit_list_counts),
// then the insertion.
template <uint32_t N>
RT_DEV void nearest_candidate(float4 a, float4 b, float2 c2, Trav& T, HitList<N>& x) {
    const float p[3] = {T.o.x, T.o.y, T.o.z};
    const float v0[3] = {a.x, a.y, a.z}, e1[3] = {a.w, b.x, b.y}, e2[3] = {b.z, b.w, c2.x};
    const uint32_t gidx = __float_as_uint(c2.y);
    const ClosestPoint cand = closest_point_on_record(p, v0, e1, e2);
    if (hit_list_counts(x, closest_better(cand.dist2, gidx, T.best.t, T.best.tri), cand.dist2, gidx))
        hit_list_insert<N>(x, T.best, Hit{cand.dist2, cand.u, cand.v, gidx});
}

// query_frame's policy (rt_query_frame.h): an entry is a point, its max_dist2 and its key — the point inside the contract's range,
// max_dist2 and after_dist2 no NaN; a step is one wave-uniform step kind by the ray traversal's vote on trav_classes (vote_step),
// closest_inner unchanged or the whole-leaf step with this unit's candidate.
struct NearestPhase {};
template <uint32_t N>
struct NearestFrame {
    static constexpr uint32_t kBlock = kNearestBlock, kRefill = kNearestRefill;
    using Lane = HitList<N>;
    RT_DEV static HitListOut out(const NearestDev& q) { return HitListOut{q.dist2, q.u, q.v, q.tri, q.count, q.k}; }
    RT_DEV static bool start(const NearestDev& q, uint32_t i, Trav& T, const TravStack& stack) {
        const size_t k = 3 * (size_t)i;
        const f3 p = mk3(q.pos[k], q.pos[k + 1], q.pos[k + 2]);
        const float inf = __builtin_huge_valf();
        const float md = q.max_dist2 ? q.max_dist2[i] : inf;
        const float ad = q.after_dist2 ? q.after_dist2[i] : -inf;
        if (in_contract_range(q.range, p.x, p.y, p.z) && md == md && ad == ad) {
            closest_begin(T, p, md, stack);
            hit_list_carry(T, ad, q.after_dist2 ? q.after_tri[i] : 0u, q.k);
            return true;
        }
        hit_list_reject(out(q), i);
        return false;
    }
    RT_DEV static NearestPhase phase(const Trav&) { return {}; }
    RT_DEV static void step(const SceneDev& S, Trav& T, Lane& x, const TravStack& stack, const TopTree& top, NearestPhase) {
        vote_step(T, [&] {
            if (T.cur == 0) hit_list_open(T, x); // a lane is at the root exactly once, in its first step
            closest_inner(S, T, stack, top);
        }, [&] { whole_leaf(S, T, stack, [&](float4 a, float4 b, float2 c2) { nearest_candidate<N>(a, b, c2, T, x); }); });
    }
    RT_DEV static void store(const NearestDev& q, uint32_t i, const Trav& T, const Lane& x) { hit_list_store<N>(out(q), i, T.best, x); }
};

template <uint32_t N>
__global__ void __launch_bounds__(kNearestBlock, kNearestWaves<N>) k_nearest(SceneDev S, NearestDev q) { query_frame<NearestFrame<N>>(S, q); }

} // namespace rt

namespace {

// the refusals, in rt_trace_rays' order (rt_query.hip: query_check)
int nearest_check(const rt_scene* s, const rt_nearest_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->n == 0) return RT_OK;
    if (q->k < 1 || q->k > RT_NEAREST_MAX) return fail(RT_ERR_INVALID, "k must be 1 .. " + std::to_string(RT_NEAREST_MAX));
    if (!q->pos) return fail(RT_ERR_INVALID, "null pos");
    if (!q->after_dist2 != !q->after_tri) return fail(RT_ERR_INVALID, "a resume key is after_dist2 and after_tri, both or neither");
    if (!q->dist2 && !q->u && !q->v && !q->tri && !q->count) return fail(RT_ERR_INVALID, "k-nearest query with every output NULL");
    return refuse_host_only(s);
}

// fills the launch struct and hands it to the list kinds' launch (PRE: nearest_check passed, n > 0, pointers on the scene's device)
int nearest_enqueue(rt_scene* s, const rt_nearest_query* q, hipStream_t st) {
    NearestDev d{};
    d.pos = q->pos, d.max_dist2 = q->max_dist2, d.after_dist2 = q->after_dist2, d.after_tri = q->after_tri;
    d.dist2 = q->dist2, d.u = q->u, d.v = q->v, d.tri = q->tri, d.count = q->count;
    d.n = q->n, d.k = q->k;
    return list_launch<kQueryKindNearest>(s, [](auto n) { return k_nearest<decltype(n)::value>; }, kNearestBlock, d, st, dev_knob("RT_NEAREST_GRID"));
}

} // namespace

extern "C" {

int rt_closest_points_multi(rt_scene* s, const rt_nearest_query* q) {
    if (const int rc = nearest_check(s, q)) return rc;
    const uint32_t n = q->n, k = q->k;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < n; ++i) {
        const float* p = q->pos + 3 * (size_t)i;
        if (!in_contract_range(range, p[0], p[1], p[2]))
            return fail(RT_ERR_INVALID, "point " + std::to_string(i) + ": more than 100 scene scales outside the scene's bounds or not finite (outside the range of the closest-point contract)");
        if (q->max_dist2 && std::isnan(q->max_dist2[i])) return fail(RT_ERR_INVALID, "point " + std::to_string(i) + ": max_dist2 is NaN");
        if (q->after_dist2 && std::isnan(q->after_dist2[i])) return fail(RT_ERR_INVALID, "point " + std::to_string(i) + ": after_dist2 is NaN");
    }
    const StageIn ins[4] = {{q->pos, 12}, {q->max_dist2, 4}, {q->after_dist2, 4}, {q->after_tri, 4}};
    StageOut outs[5];
    list_stage_outs(outs, k, q->dist2, q->u, q->v, q->tri, q->count);
    return query_staged(s, n, ins, outs, [&](void* const* in, void* const* out) {
        rt_nearest_query d{};
        d.n = n, d.k = k;
        d.pos = (const float*)in[0], d.max_dist2 = (const float*)in[1], d.after_dist2 = (const float*)in[2], d.after_tri = (const uint32_t*)in[3];
        d.dist2 = (float*)out[0], d.u = (float*)out[1], d.v = (float*)out[2], d.tri = (uint32_t*)out[3], d.count = (uint32_t*)out[4];
        return nearest_enqueue(s, &d, 0);
    });
}

int rt_closest_points_multi_device(rt_scene* s, const rt_nearest_query* q, void* stream) {
    if (const int rc = nearest_check(s, q)) return rc;
    if (q->n == 0) return RT_OK;
    return nearest_enqueue(s, q, (hipStream_t)stream);
}

int rt_scene_nearest_host(const rt_scene* s, uint32_t n, uint32_t k, const float* pos, const float* max_dist2, const float* after_dist2,
                          const uint32_t* after_tri, int use_bvh, float* dist2, float* u, float* v, uint32_t* tri, uint32_t* count,
                          uint64_t* node_visits, uint64_t* tri_tests) {
    if (!s || (n && !pos)) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc0 = sync_host_copy(s)) return rc0;
    std::string err;
    const int rc = no_throw([&] { return nearest_host(s->hs, n, k, pos, max_dist2, after_dist2, after_tri, use_bvh, dist2, u, v, tri, count, node_visits, tri_tests, err); });
    return rc == RT_OK ? RT_OK : fail(rc, err.empty() ? g_err : err);
}

} // extern "C"
