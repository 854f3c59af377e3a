// rt_closest.hip — closest-point queries: rt_closest_points[_device], the nearest triangle to caller-supplied points, their kernel k_closest
// and the C entry of the host diagnostic rt_scene_closest_host (the walk itself: scene_check.cpp: closest_host).
// (A unit of its own, as rt_query.hip is: the render kernels' listings do not change. The contract — the fp32 text of one candidate, the
// winner rule and the cull — is rt_closest_point.h, shared with the host walk. DESIGN.md §22.)
// The kernel's body is query_frame (rt_query_frame.h), shared with k_query, with the claim every query kernel shares; the launch and the host
// form's staging are rt_query_launch.h's; the start of a lane's traversal and the inner step are rt_closest_step.h's, shared with
// rt_nearest.hip; the whole-leaf read is rt_whole_leaf.h's. What is this unit's own: an entry is a point with a max_dist2, and the
// candidate of the leaf step.
#include "rt_query_launch.h"
#include "rt_query_frame.h"
#include "rt_closest_point.h"
#include "rt_closest_step.h"
#include "rt_whole_leaf.h"

namespace rt {

constexpr uint32_t kClosestBlock = 512; // threads per workgroup: 8 independent waves share one LDS copy of the top of the BVH (as k_query)
constexpr uint32_t kClosestWaves = 6;   // waves per SIMD the kernel is compiled for: three workgroups' LDS fill a CU (46,400 bytes each)
constexpr uint32_t kClosestRefill = 16; // idle lanes of a wave that end its traversal phase: they write their results and take new points

// what a launch reads and writes (include/rt_mi355x.h: rt_point_query; NULL outputs are not written)
struct PointDev {
    const float* pos;
    const float* max_dist2;
    float* dist2;
    float* u;
    float* v;
    uint32_t* tri;
    float* point;
    unsigned long long* cursor; // kQueryHeads shard cursors, kQueryHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

// one candidate: the contract's text on the record's ten live dwords, then the winner rule
RT_DEV void closest_test_regs(float4 a, float4 b, float2 c, Trav& T, f3& r) {
    const float p[3] = {T.o.x, T.o.y, T.o.z};
    const float v0[3] = {a.x, a.y, a.z}, e1[3] = {a.w, b.x, b.y}, e2[3] = {b.z, b.w, c.x};
    const uint32_t gidx = __float_as_uint(c.y);
    const ClosestPoint cand = closest_point_on_record(p, v0, e1, e2);
    if (closest_better(cand.dist2, gidx, T.best.t, T.best.tri)) {
        T.best.t = cand.dist2, T.best.u = cand.u, T.best.v = cand.v, T.best.tri = gidx;
        r = mk3(cand.r[0], cand.r[1], cand.r[2]);
    }
}

// query_frame's policy (rt_query_frame.h): an entry is a point and its max_dist2, the point inside the contract's range and max_dist2 no
// NaN; a step is one wave-uniform step kind, an inner or a leaf step, by the ray traversal's vote on trav_classes (rt_whole_leaf.h: vote_step).
// A popped child is not tested against the winner again (the stack holds words, no keys): its node is visited, and there its children
// meet the current best.
struct PointPhase {};
struct PointFrame {
    static constexpr uint32_t kBlock = kClosestBlock, kRefill = kClosestRefill;
    struct Lane { f3 r; }; // p - point of the winner
    RT_DEV static bool start(const PointDev& q, uint32_t i, Trav& T, const TravStack& stack) {
        const size_t k = 3 * (size_t)i;
        const f3 p = mk3(q.pos[k], q.pos[k + 1], q.pos[k + 2]);
        const float md = q.max_dist2 ? q.max_dist2[i] : __builtin_huge_valf();
        if (in_contract_range(q.range, p.x, p.y, p.z) && md == md) {
            closest_begin(T, p, md, stack);
            return true;
        }
        if (q.dist2) q.dist2[i] = __builtin_nanf(""); // rejected: marked, never walked
        if (q.tri) q.tri[i] = RT_TRI_REJECTED;
        return false;
    }
    RT_DEV static PointPhase phase(const Trav&) { return {}; }
    RT_DEV static void step(const SceneDev& S, Trav& T, Lane& x, const TravStack& stack, const TopTree& top, PointPhase) {
        vote_step(T, [&] { closest_inner(S, T, stack, top); },
                  [&] { whole_leaf(S, T, stack, [&](float4 a, float4 b, float2 c2) { closest_test_regs(a, b, c2, T, x.r); }); });
    }
    RT_DEV static void store(const PointDev& q, uint32_t i, const Trav& T, const Lane& x) {
        const bool hit = T.best.tri != kNoTri;
        const float nan = __builtin_nanf("");
        const size_t k = 3 * (size_t)i;
        if (q.dist2) q.dist2[i] = hit ? T.best.t : __builtin_huge_valf(); // a miss: best.t still holds max_dist2
        if (q.u) q.u[i] = T.best.u;
        if (q.v) q.v[i] = T.best.v;
        if (q.tri) q.tri[i] = T.best.tri;
        if (q.point) {
            q.point[k] = hit ? T.o.x - x.r.x : nan;
            q.point[k + 1] = hit ? T.o.y - x.r.y : nan;
            q.point[k + 2] = hit ? T.o.z - x.r.z : nan;
        }
    }
};

__global__ void __launch_bounds__(kClosestBlock, kClosestWaves) k_closest(SceneDev S, PointDev q) { query_frame<PointFrame>(S, q); }

} // namespace rt

namespace {

// the refusals, in rt_trace_rays' order (rt_query.hip: query_check)
int point_check(const rt_scene* s, const rt_point_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->n == 0) return RT_OK;
    if (!q->pos) return fail(RT_ERR_INVALID, "null pos");
    if (!q->dist2 && !q->u && !q->v && !q->tri && !q->point) return fail(RT_ERR_INVALID, "closest-point query with every output NULL");
    return refuse_host_only(s);
}

// fills the launch struct and hands it to the shared launch (PRE: point_check passed, n > 0, pointers on the scene's device)
int point_enqueue(rt_scene* s, const rt_point_query* q, hipStream_t st) {
    PointDev d{};
    d.pos = q->pos, d.max_dist2 = q->max_dist2;
    d.dist2 = q->dist2, d.u = q->u, d.v = q->v, d.tri = q->tri, d.point = q->point;
    d.n = q->n;
    return query_launch(s, kQueryKindPoint, k_closest, kClosestBlock, d, q->n, st, s->query_grid[kQueryKindPoint] ? nullptr : dev_knob("RT_CLOSEST_GRID"));
}

} // namespace

extern "C" {

int rt_closest_points(rt_scene* s, const rt_point_query* q) {
    if (const int rc = point_check(s, q)) return rc;
    const uint32_t n = q->n;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < n; ++i) {
        const float* p = q->pos + 3 * (size_t)i;
        if (!in_contract_range(range, p[0], p[1], p[2]))
            return fail(RT_ERR_INVALID, "point " + std::to_string(i) + ": more than 100 scene scales outside the scene's bounds or not finite (outside the range of the closest-point contract)");
        if (q->max_dist2 && std::isnan(q->max_dist2[i])) return fail(RT_ERR_INVALID, "point " + std::to_string(i) + ": max_dist2 is NaN");
    }
    const StageIn ins[2] = {{q->pos, 12}, {q->max_dist2, 4}};
    const StageOut outs[5] = {{q->dist2, 4}, {q->u, 4}, {q->v, 4}, {q->tri, 4}, {q->point, 12}};
    return query_staged(s, n, ins, outs, [&](void* const* in, void* const* out) {
        rt_point_query d{};
        d.n = n, d.pos = (const float*)in[0], d.max_dist2 = (const float*)in[1];
        d.dist2 = (float*)out[0], d.u = (float*)out[1], d.v = (float*)out[2], d.tri = (uint32_t*)out[3], d.point = (float*)out[4];
        return point_enqueue(s, &d, 0);
    });
}

int rt_closest_points_device(rt_scene* s, const rt_point_query* q, void* stream) {
    if (const int rc = point_check(s, q)) return rc;
    if (q->n == 0) return RT_OK;
    return point_enqueue(s, q, (hipStream_t)stream);
}

int rt_scene_closest_host(const rt_scene* s, uint32_t n, const float* pos, const float* max_dist2, int use_bvh, float* dist2, float* u, float* v,
                          uint32_t* tri, float* point, uint64_t* node_visits, uint64_t* tri_tests) {
    if (!s || (n && !pos)) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc0 = sync_host_copy(s)) return rc0;
    std::string err;
    const int rc = no_throw([&] { return closest_host(s->hs, n, pos, max_dist2, use_bvh, dist2, u, v, tri, point, node_visits, tri_tests, err); });
    return rc == RT_OK ? RT_OK : fail(rc, err.empty() ? g_err : err);
}

} // extern "C"
