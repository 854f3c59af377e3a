// rt_hit_list.h — the sorted list in registers of the k-nearest query kernels: rt_nearest.hip's (k_nearest<N>, triangles around a point in
// (dist2, tri) order; Hit::t holds dist2 there). It is the list of rt_multihit.hip (k_multihit<N>, hits along a ray in (t, tri) order),
// which keeps its own text of it: with this header that unit's device listing did not stay the same (EXPERIMENTS.md).
// N slots in ascending (t, tri) order; slots 0 .. N - 2 are an array beside the traversal, slot N - 1 is the traversal's own T.best — the
// BOUND the inner steps cull against. The caller's k <= N live in the LAST k slots; the N - k in front hold a sentinel, (-inf, kNoTri),
// that sorts before every candidate and is never moved. A free slot holds (the entry's limit, 0, 0, kNoTri): every counting candidate sorts
// before it. Every index below is a compile-time constant after unrolling: the list lives in registers (a dynamic index would put it into
// scratch). DESIGN.md §24, §25.
#pragma once
#include "rt_device.h"

namespace rt {

RT_DEV bool hit_before(const Hit& a, const Hit& b) { return a.t < b.t || (a.t == b.t && a.tri < b.tri); }
RT_DEV Hit hit_sel(bool c, const Hit& a, const Hit& b) { return Hit{c ? a.t : b.t, c ? a.u : b.u, c ? a.v : b.v, c ? a.tri : b.tri}; }

// The insertion of a candidate c that sorts before the last slot (PRE: the caller's compare against the bound said so, and c is in no
// slot): slot i takes its left neighbour where the candidate sorts before that one, the candidate where it sorts before slot i only, and
// keeps its own otherwise; what was in slot N - 1 falls out.
// (x: the lane's state, whose member s[N - 1] holds slots 0 .. N - 2; last: slot N - 1, the traversal's T.best. The walk down the slots
// is a recursion on the slot's number, not a loop: every index is a constant where the text is instantiated, whatever gets unrolled when.)
template <uint32_t I, class L>
RT_DEV void hit_list_shift(L& x, const Hit& c, bool here) {
    if constexpr (I >= 1) {
        const bool left = hit_before(c, x.s[I - 1]);
        x.s[I] = hit_sel(left, x.s[I - 1], hit_sel(here, c, x.s[I]));
        hit_list_shift<I - 1>(x, c, left);
    } else {
        x.s[0] = hit_sel(here, c, x.s[0]);
    }
}
template <uint32_t N, class L>
RT_DEV void hit_list_insert(L& x, Hit& last, const Hit& c) {
    const bool here = hit_before(c, x.s[N - 2]); // from the last slot down: two compares are alive at a time, not N - 1
    last = hit_sel(here, x.s[N - 2], c);
    hit_list_shift<N - 2>(x, c, here);
}

} // namespace rt
