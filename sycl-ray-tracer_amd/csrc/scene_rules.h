// scene_rules.h — the scene's geometry rules, one text each for the host builder and refit (scene_build.cpp), the device update (rt_update.hip:
// k_upd_*) and the device builder (lbvh_gpu.hip: k_prims). Plain fp32 operators: every unit is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>

#include "bvh_quantise.h"
#include "rt_types.h"

namespace rt {

// Axis a of a world-space vertex: row a of the column-major instance matrix m on the object-space (x, y, z), in the oracle's order.
RT_HD float world_coord(const float* m, int a, float x, float y, float z) { return ((m[a] * x + m[4 + a] * y) + m[8 + a] * z) + m[12 + a]; }

// Boxes are reduced with fminf / fmaxf. The operands are finite (a non-finite vertex is refused first), so against std::min / std::max only
// the sign of a zero could differ, and nothing observable reads it: the quantiser adds a positive pad, the exact boxes feed surface areas only,
// and the scene's own bounds are not reduced here (world_bounds, the ordered keys of k_upd_transform: first occurrence). DESIGN.md §12.
RT_HD Box3 tri_box(const float* w) { // w: the triangle's nine world-space floats
    Box3 b;
    for (int a = 0; a < 3; ++a) b.lo[a] = fminf(w[a], fminf(w[3 + a], w[6 + a])), b.hi[a] = fmaxf(w[a], fmaxf(w[3 + a], w[6 + a]));
    return b;
}
RT_HD Box3 empty_box() { return {{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}}; }
RT_HD void grow(Box3& b, const Box3& c) {
    for (int a = 0; a < 3; ++a) b.lo[a] = fminf(b.lo[a], c.lo[a]), b.hi[a] = fmaxf(b.hi[a], c.hi[a]);
}

// A leaf record's v0, e1 = v1 - v0, e2 = v2 - v0 from its triangle's nine floats (part of the contract too: the kernels intersect these).
RT_HD void tri_record(const float* w, float* v0, float* e1, float* e2) {
    for (int a = 0; a < 3; ++a) v0[a] = w[a], e1[a] = w[3 + a] - w[a], e2[a] = w[6 + a] - w[a];
}

// ShadeRec::instance: the instance's table row with its material in the high bits where the word is packed (rt_types.h), else its index.
RT_HD uint32_t shading_word(bool packed, uint32_t slot, uint32_t material, uint32_t instance) {
    return packed ? (slot | (material << kPackedInstBits)) : instance;
}

// The three shading normals of a triangle, gathered through its vertex indices.
RT_HD void shade_normals(ShadeRec& s, const uint32_t* idx3, const float* normals) {
    float* dst[3] = {s.n0, s.n1, s.n2};
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) dst[k][a] = normals[3 * (size_t)idx3[k] + a];
}

// The refit of one node. inner_box(child word): the exact box an inner child stored earlier (a node's children lie in lower height levels);
// tri_of(r): the nine floats of leaf record r's triangle (a leaf's exact box: the union of its records' whole triangles). u receives the
// children's union, q the node with words 0..11 re-quantised under `pad`, child words kept. Empty: nothing written; refused: q written all the same.
enum RefitResult : int { kRefitEmpty = 0, kRefitDone = 1, kRefitRefused = 2 };
template <typename InnerBox, typename TriOf>
RT_HD RefitResult refit_node(const BvhNode& nd, InnerBox inner_box, TriOf tri_of, float pad, Box3& u, BvhNode& q) {
    Box3 kb[4];
    int nk = 0;
    for (int k = 0; k < 4 && nd.child[k] != kChildEmpty; ++k, ++nk) {
        const LeafRange leaf = leaf_range(nd.child[k]);
        kb[k] = nd.child[k] >= 0 ? inner_box(nd.child[k]) : empty_box();
        for (uint32_t r = leaf.first; nd.child[k] < 0 && r < leaf.first + leaf.count; ++r) grow(kb[k], tri_box(tri_of(r)));
    }
    if (nk == 0) return kRefitEmpty;
    Box3 b = kb[0];
    for (int k = 1; k < nk; ++k) grow(b, kb[k]);
    u = b; // (the device hands in the node's slot of its box array: stored here, the six floats are not held in registers across the quantiser)
    const bool ok = quantise_node(q, nk, kb, pad);
    for (int k = 0; k < 4; ++k) q.child[k] = nd.child[k];
    return ok ? kRefitDone : kRefitRefused;
}

} // namespace rt
