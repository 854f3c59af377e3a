// rt_multihit.hip — multi-hit ray queries: rt_trace_rays_multi[_device], the k nearest counting hits of every ray in (t, index) order,
// resumable with a key; their kernel k_multihit<N> and the C entry of the host diagnostic rt_scene_multihit_host (the walk itself:
// scene_check.cpp: multihit_host).
// (A unit of its own, as rt_query.hip and rt_closest.hip are: the render kernels' listings do not change. DESIGN.md §24.)
// The kernel's body is query_frame (rt_query_frame.h) with the claim every query kernel shares; the launch and the host form's staging are
// rt_query_launch.h's. No arithmetic of the traversal is restated here: the inner step is trav_inner, the candidate is tri_test_regs, the
// classes are trav_classes', the vote on them is rt_whole_leaf.h's vote_step. What is this unit's own: an entry is a ray with a tmax and a key, T.best is
// not the answer but the BOUND, and the leaf step keeps a sorted list of N hits in registers — the list's state, its opening, its
// key-and-duplicate test and its store are rt_hit_list.h's, the whole-leaf read is rt_whole_leaf.h's; the insertion loop is this unit's.
// What it relies on in rt_device.h, whose text it does not edit (held by tests/test_multihit.py:
// test_what_the_kernel_relies_on_in_the_traversal): cur == 0 only in a ray's first step (trav_begin alone sets it, no node has the root
// as a child), and trav_inner reads nothing of T.best but best.t — so k and the key can travel in best.u / v / tri to that first step.
#include "rt_query_launch.h"
#include "rt_query_frame.h"
#include "rt_hit_list.h"
#include "rt_whole_leaf.h"

namespace rt {

constexpr uint32_t kMultiBlock = 512; // threads per workgroup: 8 independent waves share one LDS copy of the top of the BVH (as k_query)
constexpr uint32_t kMultiRefill = 16; // idle lanes of a wave that end its traversal phase: they write their results and take new rays
// waves per SIMD an instantiation is compiled for: a list of N slots is 4 N registers beside the traversal's. Two slots fit k_query's
// budget (6 waves, 80 VGPRs: 74 used); four at 6 waves spill 4 VGPRs (and three spill 2), so the 4- and 8-slot lists are compiled for 4
// waves (two workgroups per CU: 104 and 123 VGPRs, none spilled). DESIGN.md §24: the resources per instantiation.
template <uint32_t N> constexpr uint32_t kMultiWaves = N > 2 ? 4 : 6;

// what a launch reads and writes (include/rt_mi355x.h: rt_multihit_query; NULL outputs are not written)
struct MultiDev {
    const float* org;
    const float* dir;
    const float* tmax;
    const float* after_t;
    const uint32_t* after_tri;
    float* t;
    float* u;
    float* v;
    uint32_t* tri;
    uint32_t* count;
    unsigned long long* cursor; // kQueryHeads shard cursors, kQueryHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n, k;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

// THE LIST is rt_hit_list.h's: the k-th entry is slot N - 1 whatever k is, and slot N - 1 IS T.best: the traversal's closest hit so far
// is the list's last entry, the bound. A free slot holds (tmax, 0, 0, kNoTri): every counting candidate sorts before it (t <= tmax,
// index < kNoTri), so filling the list and replacing its last entry are one insertion, and the
// bound is (tmax, kNoTri) while a slot is free and (t, tri) of the k-th entry once none is — by tri_test_regs' own compare, t < best.t
// or t == best.t at a lower index, a candidate is written exactly when it counts against tmax and sorts before the k-th entry.
// trav_inner culls child boxes against best.t and keeps boxes at equal distance: a candidate that ties with the k-th entry at a lower
// index is still reached (§14's tmax argument on a moving bound).

// One candidate: the contract's test on a copy of the bound, the key and the de-duplication (hit_list_counts), then the insertion: slot i
// takes its left neighbour where the candidate sorts before that one, the candidate where it sorts before slot i only, and keeps its own
// otherwise; what was in slot N - 1 falls out. (This unit's own loop, not hit_list_insert: rt_hit_list.h says why.)
template <uint32_t N>
RT_DEV void multi_candidate(float4 a, float4 b, float2 c2, Trav& T, HitList<N>& x) {
    Hit c = T.best;
    tri_test_regs(a, b, c2, T.o, T.d, c);
    // written: a candidate never has the bound's index (kNoTri, or an entry's: that one ties, and a tie is no win)
    if (hit_list_counts(x, c.tri != T.best.tri, c.t, c.tri)) {
        bool here = hit_before(c, x.s[N - 2]); // from the last slot down: two compares are alive at a time, not N - 1
        T.best = hit_sel(here, x.s[N - 2], c);
#pragma unroll
        for (uint32_t i = N - 2; i >= 1; --i) {
            const bool left = hit_before(c, x.s[i - 1]);
            x.s[i] = hit_sel(left, x.s[i - 1], hit_sel(here, c, x.s[i]));
            here = left;
        }
        x.s[0] = hit_sel(here, c, x.s[0]);
    }
}

// query_frame's policy (rt_query_frame.h): an entry is a ray, its tmax and its key — the origin inside the contract's range, tmax and
// after_t no NaN; a step is one wave-uniform step kind by the ray traversal's vote on trav_classes (vote_step),
// trav_inner unchanged or the whole-leaf step with this unit's candidate.
template <uint32_t N>
struct HitsFrame {
    static constexpr uint32_t kBlock = kMultiBlock, kRefill = kMultiRefill;
    using Lane = HitList<N>;
    RT_DEV static HitListOut out(const MultiDev& q) { return HitListOut{q.t, q.u, q.v, q.tri, q.count, q.k}; }
    RT_DEV static bool start(const MultiDev& q, uint32_t i, Trav& T, const TravStack& stack) {
        const size_t k = 3 * (size_t)i;
        const f3 o = mk3(q.org[k], q.org[k + 1], q.org[k + 2]);
        const f3 d = mk3(q.dir[k], q.dir[k + 1], q.dir[k + 2]);
        const float inf = __builtin_huge_valf();
        const float tm = q.tmax ? q.tmax[i] : inf;
        const float at = q.after_t ? q.after_t[i] : -inf;
        if (in_contract_range(q.range, o.x, o.y, o.z) && tm == tm && at == at) {
            trav_begin(T, o, d, stack);
            T.best.t = tm;
            hit_list_carry(T, at, q.after_t ? q.after_tri[i] : 0u, q.k); // (the bound's index is not read before the first leaf step)
            return true;
        }
        hit_list_reject(out(q), i);
        return false;
    }
    RT_DEV static TravSigns phase(const Trav& T) { return trav_signs(T); }
    RT_DEV static void step(const SceneDev& S, Trav& T, Lane& x, const TravStack& stack, const TopTree& top, const TravSigns& sg) {
        vote_step(T, [&] {
            if (T.cur == 0) hit_list_open(T, x); // a lane is at the root exactly once, in its first step
            trav_inner(S, T, stack, top, sg);
        }, [&] { whole_leaf(S, T, stack, [&](float4 a, float4 b, float2 c2) { multi_candidate<N>(a, b, c2, T, x); }); });
    }
    RT_DEV static void store(const MultiDev& q, uint32_t i, const Trav& T, const Lane& x) { hit_list_store<N>(out(q), i, T.best, x); }
};

template <uint32_t N>
__global__ void __launch_bounds__(kMultiBlock, kMultiWaves<N>) k_multihit(SceneDev S, MultiDev q) { query_frame<HitsFrame<N>>(S, q); }

} // namespace rt

namespace {

// the refusals, in rt_trace_rays' order (rt_query.hip: query_check)
int multi_check(const rt_scene* s, const rt_multihit_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->n == 0) return RT_OK;
    if (q->k < 1 || q->k > RT_MULTIHIT_MAX) return fail(RT_ERR_INVALID, "k must be 1 .. " + std::to_string(RT_MULTIHIT_MAX));
    if (!q->org || !q->dir) return fail(RT_ERR_INVALID, "null org or dir");
    if (!q->after_t != !q->after_tri) return fail(RT_ERR_INVALID, "a resume key is after_t and after_tri, both or neither");
    if (!q->t && !q->u && !q->v && !q->tri && !q->count) return fail(RT_ERR_INVALID, "multi-hit query with every output NULL");
    return refuse_host_only(s);
}

// fills the launch struct and hands it to the list kinds' launch (PRE: multi_check passed, n > 0, pointers on the scene's device)
int multi_enqueue(rt_scene* s, const rt_multihit_query* q, hipStream_t st) {
    MultiDev d{};
    d.org = q->org, d.dir = q->dir, d.tmax = q->tmax, d.after_t = q->after_t, d.after_tri = q->after_tri;
    d.t = q->t, d.u = q->u, d.v = q->v, d.tri = q->tri, d.count = q->count;
    d.n = q->n, d.k = q->k;
    return list_launch<kQueryKindMulti>(s, [](auto n) { return k_multihit<decltype(n)::value>; }, kMultiBlock, d, st, dev_knob("RT_MULTIHIT_GRID"));
}

} // namespace

extern "C" {

int rt_trace_rays_multi(rt_scene* s, const rt_multihit_query* q) {
    if (const int rc = multi_check(s, q)) return rc;
    const uint32_t n = q->n, k = q->k;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < n; ++i) {
        if (const int rc = refuse_ray_origin(range, q->org, i)) return rc;
        if (q->tmax && std::isnan(q->tmax[i])) return fail(RT_ERR_INVALID, "ray " + std::to_string(i) + ": tmax is NaN");
        if (q->after_t && std::isnan(q->after_t[i])) return fail(RT_ERR_INVALID, "ray " + std::to_string(i) + ": after_t is NaN");
    }
    const StageIn ins[5] = {{q->org, 12}, {q->dir, 12}, {q->tmax, 4}, {q->after_t, 4}, {q->after_tri, 4}};
    StageOut outs[5];
    list_stage_outs(outs, k, q->t, q->u, q->v, q->tri, q->count);
    return query_staged(s, n, ins, outs, [&](void* const* in, void* const* out) {
        rt_multihit_query d{};
        d.n = n, d.k = k;
        d.org = (const float*)in[0], d.dir = (const float*)in[1], d.tmax = (const float*)in[2];
        d.after_t = (const float*)in[3], d.after_tri = (const uint32_t*)in[4];
        d.t = (float*)out[0], d.u = (float*)out[1], d.v = (float*)out[2], d.tri = (uint32_t*)out[3], d.count = (uint32_t*)out[4];
        return multi_enqueue(s, &d, 0);
    });
}

int rt_trace_rays_multi_device(rt_scene* s, const rt_multihit_query* q, void* stream) {
    if (const int rc = multi_check(s, q)) return rc;
    if (q->n == 0) return RT_OK;
    return multi_enqueue(s, q, (hipStream_t)stream);
}

int rt_scene_multihit_host(const rt_scene* s, uint32_t n, uint32_t k, const float* org, const float* dir, const float* tmax, const float* after_t,
                           const uint32_t* after_tri, int use_bvh, float* t, float* u, float* v, uint32_t* tri, uint32_t* count,
                           uint64_t* node_visits, uint64_t* tri_tests) {
    if (!s || (n && (!org || !dir))) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc0 = sync_host_copy(s)) return rc0;
    std::string err;
    const int rc = no_throw([&] { return multihit_host(s->hs, n, k, org, dir, tmax, after_t, after_tri, use_bvh, t, u, v, tri, count, node_visits, tri_tests, err); });
    return rc == RT_OK ? RT_OK : fail(rc, err.empty() ? g_err : err);
}

} // extern "C"
