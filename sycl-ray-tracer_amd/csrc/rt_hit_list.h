// rt_hit_list.h — the sorted list in registers of the k-list query kernels: rt_multihit.hip (k_multihit<N>, hits along a ray in (t, tri)
// order) and rt_nearest.hip (k_nearest<N>, triangles around a point in (dist2, tri) order; Hit::t holds dist2 there, and the entry's limit
// is tmax or max_dist2).
// SHARED, one text for both units: the lane's state (HitList<N>), the order (hit_before, hit_sel), the carry of k and the key to the
// lane's first step (hit_list_carry), the opening at the root (hit_list_open), the key-and-duplicate test (hit_list_counts), the outputs
// with the marking of a rejected entry and the store (HitListOut, hit_list_reject, hit_list_store).
// NOT shared: the insertion. hit_list_insert below is k_nearest's; rt_multihit.hip keeps its own loop over the same hit_before / hit_sel,
// because with hit_list_insert that unit's device listing did not stay the same (EXPERIMENTS.md).
// N slots in ascending (t, tri) order; slots 0 .. N - 2 are an array beside the traversal, slot N - 1 is the traversal's own T.best — the
// BOUND the inner steps cull against. The caller's k <= N live in the LAST k slots; the N - k in front hold a sentinel, (-inf, kNoTri),
// that sorts before every candidate and is never moved. A free slot holds (the entry's limit, 0, 0, kNoTri): every counting candidate sorts
// before it. Every index below is a compile-time constant after unrolling: the list lives in registers (a dynamic index would put it into
// scratch). DESIGN.md §24, §25.
#pragma once
#include "rt_device.h"

namespace rt {

template <uint32_t N>
struct HitList {
    Hit s[N - 1];       // slots 0 .. N - 2; slot N - 1 is T.best
    float after_t;      // the key: a candidate counts iff (t, tri) > (after_t, after_tri); no key = (-inf, 0), below every candidate
    uint32_t after_tri;
};

RT_DEV bool hit_before(const Hit& a, const Hit& b) { return a.t < b.t || (a.t == b.t && a.tri < b.tri); }
RT_DEV Hit hit_sel(bool c, const Hit& a, const Hit& b) { return Hit{c ? a.t : b.t, c ? a.u : b.u, c ? a.v : b.v, c ? a.tri : b.tri}; }

// query_frame hands a policy's start() the lane's Trav, not its list: k and the key travel in T.best.u / v / tri — the inner steps read
// best.t alone — to the lane's first step, the one at the root (cur == 0 exactly once), which opens the list: the key taken out of T.best,
// the sentinels and the free slots written (best.t holds the entry's limit), the bound's own slot set free.
RT_DEV void hit_list_carry(Trav& T, float after_t, uint32_t after_tri, uint32_t k) { T.best.u = after_t, T.best.v = __uint_as_float(after_tri), T.best.tri = k; }
template <uint32_t N>
RT_DEV void hit_list_open(Trav& T, HitList<N>& x) {
    const uint32_t k = T.best.tri;
    x.after_t = T.best.u, x.after_tri = __float_as_uint(T.best.v);
#pragma unroll
    for (uint32_t s = 0; s + 1 < N; ++s) x.s[s] = Hit{s + k < N ? -__builtin_huge_valf() : T.best.t, 0.0f, 0.0f, kNoTri};
    T.best.u = T.best.v = 0.0f, T.best.tri = kNoTri;
}

// `take` (the candidate passed the unit's compare against the bound, slot N - 1) and the key and the de-duplication against the other
// slots: a pre-split triangle sits whole in several leaves and gives the same bits each time
template <uint32_t N>
RT_DEV bool hit_list_counts(const HitList<N>& x, bool take, float t, uint32_t tri) {
    take = take && (t > x.after_t || (t == x.after_t && tri > x.after_tri));
#pragma unroll
    for (uint32_t i = 0; i + 1 < N; ++i) take = take && tri != x.s[i].tri;
    return take;
}

// The insertion of a candidate c that sorts before the last slot (PRE: the caller's compare against the bound said so, and c is in no
// slot): slot i takes its left neighbour where the candidate sorts before that one, the candidate where it sorts before slot i only, and
// keeps its own otherwise; what was in slot N - 1 falls out.
// (last: slot N - 1, the traversal's T.best. The walk down the slots is a recursion on the slot's number, not a loop: every index is a
// constant where the text is instantiated, whatever gets unrolled when.)
template <uint32_t I, uint32_t N>
RT_DEV void hit_list_shift(HitList<N>& x, const Hit& c, bool here) {
    if constexpr (I >= 1) {
        const bool left = hit_before(c, x.s[I - 1]);
        x.s[I] = hit_sel(left, x.s[I - 1], hit_sel(here, c, x.s[I]));
        hit_list_shift<I - 1>(x, c, left);
    } else {
        x.s[0] = hit_sel(here, c, x.s[0]);
    }
}
template <uint32_t N>
RT_DEV void hit_list_insert(HitList<N>& x, Hit& last, const Hit& c) {
    const bool here = hit_before(c, x.s[N - 2]); // from the last slot down: two compares are alive at a time, not N - 1
    last = hit_sel(here, x.s[N - 2], c);
    hit_list_shift<N - 2>(x, c, here);
}

// what a list kernel writes, entry-major, k slots per entry (NULL: not written); t is the unit's t or dist2
struct HitListOut {
    float* t;
    float* u;
    float* v;
    uint32_t* tri;
    uint32_t* count;
    uint32_t k;
};

// a rejected entry: every slot marked, never walked
RT_DEV void hit_list_reject(const HitListOut& q, uint32_t i) {
    for (uint32_t j = 0; j < q.k; ++j) {
        if (q.t) q.t[(size_t)i * q.k + j] = __builtin_nanf("");
        if (q.tri) q.tri[(size_t)i * q.k + j] = RT_TRI_REJECTED;
    }
    if (q.count) q.count[i] = 0u;
}

// slot s of the list is output slot s - (N - k) of the entry; a slot nothing was inserted into still has kNoTri and is written as a miss
template <uint32_t N>
RT_DEV void hit_list_store_slot(const HitListOut& q, uint32_t i, uint32_t s, const Hit& h, uint32_t& filled) {
    if (s + q.k < N) return;
    const size_t at = (size_t)i * q.k + (s + q.k - N);
    const bool hit = h.tri != kNoTri;
    filled += hit ? 1u : 0u;
    if (q.t) q.t[at] = hit ? h.t : __builtin_huge_valf(); // a free slot: t still holds the entry's limit
    if (q.u) q.u[at] = h.u;
    if (q.v) q.v[at] = h.v;
    if (q.tri) q.tri[at] = h.tri;
}
template <uint32_t N>
RT_DEV void hit_list_store(const HitListOut& q, uint32_t i, const Hit& last, const HitList<N>& x) {
    uint32_t filled = 0u;
#pragma unroll
    for (uint32_t s = 0; s + 1 < N; ++s) hit_list_store_slot<N>(q, i, s, x.s[s], filled);
    hit_list_store_slot<N>(q, i, N - 1, last, filled);
    if (q.count) q.count[i] = filled;
}

} // namespace rt
