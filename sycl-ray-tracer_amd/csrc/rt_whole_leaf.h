// rt_whole_leaf.h — the vote on the step kind and the whole-leaf read of the query kernels that bring their own candidate: rt_closest.hip (k_closest), rt_nearest.hip
// (k_nearest<N>) and rt_multihit.hip (k_multihit<N>). rt_device.h's trav_leaf<true> holds the same read with the ray test built in; that
// text is the render kernels' and stays where it is. DESIGN.md §22, §24, §25.
#pragma once
#include "rt_device.h"

namespace rt {

// Leaf step: the whole leaf (1-2 records) as trav_leaf<true> reads it — five unconditional 16-byte loads of 80 contiguous bytes (a leaf of
// one record reads 40 bytes of its neighbour and ignores them; the buffer ends in 48 bytes of padding) — then one or two candidates,
// cand(a, b, c2) on a record's ten live dwords, the second under a ballot; then the pop.
template <class Cand>
RT_DEV void whole_leaf(const SceneDev& S, Trav& T, const TravStack& stack, Cand cand) {
    static_assert(kMaxLeafTris == 2 && kTriBytes == 40, "the whole-leaf step reads a leaf as 80 contiguous bytes");
    const uint32_t code = (uint32_t)~T.cur;
    const uint32_t first = code >> 2, rem = code & 3u;
    const uint8_t* p4 = S.tris + (size_t)first * kTriBytes;
    const float4 l0 = tri_ld4(p4), l1 = tri_ld4(p4 + 16), l2 = tri_ld4(p4 + 32), l3 = tri_ld4(p4 + 48), l4 = tri_ld4(p4 + 64);
    const bool two = rem != 0u;
    cand(l0, l1, make_float2(l2.x, l2.y));
    if (__ballot(two) != 0ull) {
        if (two) cand(make_float4(l2.z, l2.w, l3.x, l3.y), make_float4(l3.z, l3.w, l4.x, l4.y), make_float2(l4.z, l4.w));
    }
    if (lanes(!stack_shallow(stack, T, 0u)) == 0ull) trav_pop_lds(T, stack);
    else trav_pop(T, stack);
}

// One wave-uniform step kind by the ray traversal's vote on trav_classes (trav_step_wave<.., LEAF_BATCH>'s line, which cannot be called:
// that function calls its own leaf step): inner() in the lanes at an inner node, or leaf() in the lanes at a leaf.
template <class Inner, class Leaf>
RT_DEV void vote_step(const Trav& T, Inner inner, Leaf leaf) {
    const TravClasses c = trav_classes(T);
    const uint32_t ni = count(c.inner), nl = count(c.leaf);
    if (ni * kVoteInner >= nl * kVoteLeaf && !(nl >= 64u)) {
        if (in_mask(c.inner)) inner();
    } else {
        if (in_mask(c.leaf)) leaf();
    }
}

} // namespace rt
