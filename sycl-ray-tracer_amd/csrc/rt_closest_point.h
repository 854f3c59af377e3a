// rt_closest_point.h — the contract of the closest-point queries (include/rt_mi355x.h: rt_closest_points), written once for the kernel
// (rt_closest.hip: k_closest) and for the host walk (scene_check.cpp: closest_host). DESIGN.md §22.
//
// For a point p and a leaf record (v0, e1, e2) as the kernels hold it: Ericson's region walk ("Real-Time Collision Detection", 5.1.5) on the
// record, every operation ONE fp32 operation of DESIGN.md §3 (R1), left to right as bracketed, never contracted (both users are compiled
// with -ffp-contract=off); dot is R2's unfused (ax*bx + ay*by) + az*bz; divisions are correctly rounded; no square root anywhere.
//
//     ap = p - v0;  d1 = dot(e1, ap);  d2 = dot(e2, ap)
//     bp = ap - e1; d3 = dot(e1, bp);  d4 = dot(e2, bp)
//     cp = ap - e2; d5 = dot(e1, cp);  d6 = dot(e2, cp)
//     vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4
//     the first region that holds, in this order:
//       d1 <= 0 && d2 <= 0                         (u, v) = (0, 0)
//       d3 >= 0 && d4 <= d3                        (1, 0)
//       vc <= 0 && d1 >= 0 && d3 <= 0              (d1 / (d1 - d3), 0)
//       d6 >= 0 && d5 <= d6                        (0, 1)
//       vb <= 0 && d2 >= 0 && d6 <= 0              (0, d2 / (d2 - d6))
//       va <= 0 && (d4-d3) >= 0 && (d5-d6) >= 0    w = (d4-d3) / ((d4-d3) + (d5-d6)); (1.0f - w, w)
//       else                                       den = (va + vb) + vc; (vb / den, vc / den)
//     r = (ap - u*e1) - v*e2   (per component);   dist2 = dot(r, r);   point = p - r
//
// (u, v) are barycentrics along e1 / e2, as rt_intersect_batch returns them. A triangle COUNTS iff dist2 <= max_dist2; a NaN dist2 (a
// degenerate triangle can give one: den = 0) never counts. The winner is the lowest dist2, ties to the lowest global triangle index:
// a candidate wins iff  dist2 < best || (dist2 == best && index < best_index)  from best = max_dist2, best_index = 0xFFFFFFFF
// (closest_better). The tree only culls: the result is the brute-force minimum of this expression over all triangles, bit for bit.
//
// THE LIMIT. The result is this arithmetic, not the real closest point. On slivers the point lies on the triangle (u, v >= 0, u + v <= 1 up
// to rounding) but need not be the nearest point of it: the region tests decide on products that cancel, and where |e1||e2| / |e1 x e2| is
// about 10^4 the point was measured thousands of ulp of the scene scale away from the true one. What IS bounded for every triangle, slivers
// included, is the other side —
//     sqrt(dist2) >= d_true - 8 * 2^-24 * (|ap| + |e1| + |e2|)
// (the point is a point of the triangle's plane patch computed with ~8 roundings of terms bounded by |ap| + |e1| + |e2|, and no point of the
// triangle is nearer than d_true; a numpy restatement measured at most 2.6 of the 8 on 1.2 M pairs at 1 and at 100 scene scales) — and the
// tree's cull (closest_enters) leans on this side alone.
#pragma once
#include "rt_types.h"

namespace rt {

struct ClosestPoint {
    float dist2, u, v;
    float r[3]; // p - point
};

RT_HD float closest_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

RT_HD ClosestPoint closest_point_on_record(const float p[3], const float v0[3], const float e1[3], const float e2[3]) {
    const float ap[3] = {p[0] - v0[0], p[1] - v0[1], p[2] - v0[2]};
    const float d1 = closest_dot(e1, ap), d2 = closest_dot(e2, ap);
    const float bp[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]};
    const float d3 = closest_dot(e1, bp), d4 = closest_dot(e2, bp);
    const float cp[3] = {ap[0] - e2[0], ap[1] - e2[1], ap[2] - e2[2]};
    const float d5 = closest_dot(e1, cp), d6 = closest_dot(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    float u, v;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        u = 0.0f, v = 0.0f;
    } else if (d3 >= 0.0f && d4 <= d3) {
        u = 1.0f, v = 0.0f;
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        u = d1 / (d1 - d3), v = 0.0f;
    } else if (d6 >= 0.0f && d5 <= d6) {
        u = 0.0f, v = 1.0f;
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        u = 0.0f, v = d2 / (d2 - d6);
    } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        u = 1.0f - w, v = w;
    } else {
        const float den = (va + vb) + vc;
        u = vb / den, v = vc / den;
    }
    ClosestPoint c;
    c.u = u, c.v = v;
    for (int a = 0; a < 3; ++a) c.r[a] = (ap[a] - u * e1[a]) - v * e2[a];
    c.dist2 = closest_dot(c.r, c.r);
    return c;
}

// the winner rule (a NaN dist2 fails both compares)
RT_HD bool closest_better(float dist2, uint32_t index, float best, uint32_t best_index) { return dist2 < best || (dist2 == best && index < best_index); }

// ---- the cull ---------------------------------------------------------------------------------------------------------------------------
// lb: the squared distance from p to a child's decoded box — e = max(max(lo - p, p - hi), 0) per axis, lb = e . e — cull arithmetic, free to
// fuse. The child is entered iff it exists and lb * kClosestSlack <= best. Why that never culls a triangle that could still win (DESIGN.md
// §22): the decoded box holds the subtree's triangles with at least half the builder's padding to spare (2e-5 x scene scale; check_bvh),
// so sqrt(lb) <= d_true - 1e-5 scale wherever lb > 0, and sqrt(dist2) >= d_true - 4.8e-7 (|ap| + |e1| + |e2|) (above). Near the scene the
// padding covers that error; 100 scene scales out it is five times the padding, and there the factor's 5e-5 x distance covers it.
constexpr float kClosestSlack = 0.9999f;
RT_HD bool closest_enters(float lb, float best) { return lb * kClosestSlack <= best; }

// ---- the k nearest (include/rt_mi355x.h: rt_nearest_query; rt_nearest.hip: k_nearest, scene_check.cpp: nearest_host) -------
// The same candidate, sorted. A candidate COUNTS iff dist2 <= max_dist2 and, with a resume key, (dist2, index) > (after_dist2, after_tri)
// lexicographically; a NaN dist2 never counts. The answer is the k smallest counting candidates in ascending (dist2, index) order, each
// triangle once; unfilled slots hold the miss (+inf, 0, 0, 0xFFFFFFFF). Both walks keep `best` as the BOUND: (max_dist2, 0xFFFFFFFF)
// while a slot is free, (dist2, index) of the k-th entry once none is; a candidate enters the list iff closest_better says so against the
// bound, it lies behind the key and its index is in no slot. The cull is closest_enters against that bound, unchanged: the argument above
// is about the candidate's underestimate of d_true and says nothing of where `best` came from, so it holds for every value the bound
// takes on its way down — a triangle that belongs among the k nearest has sqrt(dist2) <= sqrt(bound) at every moment of the walk, and its
// boxes are entered. The key filters candidates and culls no box.

} // namespace rt
