// rt_closest_step.h — the steps of the point traversal that the closest-point kernels share: rt_closest.hip (k_closest, the nearest
// triangle) and rt_nearest.hip (k_nearest<N>, the k nearest). One text of how a lane's traversal starts and of the inner step, with the
// cull of rt_closest_point.h (closest_enters); the leaf steps, where the two differ, stay with their units. DESIGN.md §22, §25.
#pragma once
#include "rt_query_frame.h"
#include "rt_closest_point.h"

namespace rt {

// The traversal state is the ray traversal's (rt_device.h: Trav), so that the stack helpers take it: o = the point, best.t = the winner's
// dist2 (max_dist2 until a triangle counts), best.u / v / tri = the winner's; the ray's other fields are never written or read. `r` beside
// it: p - point of the winner (the point is formed where the result is written).
RT_DEV void closest_begin(Trav& T, f3 p, float max_dist2, const TravStack& st) {
    T.o = p;
    T.best.t = max_dist2;
    T.best.u = T.best.v = 0.0f;
    T.best.tri = kNoTri;
    T.cur = 0; // root
    T.sp = stack_base(st);
}

// Inner step. The node from the LDS top or from memory (plain loads); per child the two decoded planes per axis (child_plane's value: q * s is
// exact, so the fma rounds once, as origin + q * s does), e = max(lo - p, p - hi, 0), lb = e . e (fused: cull arithmetic). A child is
// entered iff its WORD says it exists and closest_enters(lb, best): an absent child's inverted box (qlo = 255, qhi = 0) misses every ray by
// itself but gives a point a finite lb, and its word, kChildEmpty, is kTravDone — descending into it would end the lane's traversal with a
// wrong answer. A child not entered carries +inf and sinks to the end of the sorting network (five comparators: a full sort, nearest
// first; an entered child's key is clamped below +inf); the others are pushed far to near, three pushes at most, with trav_inner's
// unconditional writes where every lane of the step stays inside the LDS part of its stack.
RT_DEV void closest_inner(const SceneDev& S, Trav& T, const TravStack& stack, const TopTree& top) {
    const float inf = __builtin_huge_valf();
    u32x4 w0, w1, w2, chw;
    if (T.cur < top.count * 64) { // top of the tree: LDS, 16 bytes per node and plane
        const uint32_t o = (uint32_t)T.cur >> 2;
        w0 = *(lds_u32x4*)(size_t)((uint32_t)(size_t)top.w0 + o), w1 = *(lds_u32x4*)(size_t)((uint32_t)(size_t)top.w1 + o);
        w2 = *(lds_u32x4*)(size_t)((uint32_t)(size_t)top.w2 + o), chw = *(lds_u32x4*)(size_t)((uint32_t)(size_t)top.ch + o);
    } else {
        const u32x4* np = reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(S.nodes) + (uint32_t)T.cur);
        w0 = np[0], w1 = np[1], w2 = np[2], chw = np[3];
    }
    const float gx = __uint_as_float(w0.x), gy = __uint_as_float(w0.y), gz = __uint_as_float(w0.z);
    const float sx = __builtin_fabsf(__uint_as_float(w0.w)), sy = __builtin_fabsf(__uint_as_float(w2.z)), sz = __builtin_fabsf(__uint_as_float(w2.w));
    const float best = T.best.t;
    float k0, k1, k2, k3;
#define RT_CHILD(K, CVT, CW)                                                                              \
    {                                                                                                    \
        const float ex = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(CVT(w1.x), sx, gx) - T.o.x, T.o.x - __builtin_fmaf(CVT(w1.y), sx, gx)), 0.0f); \
        const float ey = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(CVT(w1.z), sy, gy) - T.o.y, T.o.y - __builtin_fmaf(CVT(w1.w), sy, gy)), 0.0f); \
        const float ez = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(CVT(w2.x), sz, gz) - T.o.z, T.o.z - __builtin_fmaf(CVT(w2.y), sz, gz)), 0.0f); \
        const float lb = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));                        \
        const bool enter = (int32_t)(CW) != kChildEmpty && closest_enters(lb, best);                     \
        K = sel(lanes(enter), inf, __builtin_fminf(lb, __FLT_MAX__));                                    \
    }
    RT_CHILD(k0, ub0, chw.x)
    RT_CHILD(k1, ub1, chw.y)
    RT_CHILD(k2, ub2, chw.z)
    RT_CHILD(k3, ub3, chw.w)
#undef RT_CHILD
    int32_t c0 = (int32_t)chw.x, c1 = (int32_t)chw.y, c2 = (int32_t)chw.z, c3 = (int32_t)chw.w;
#define RT_CE(KA, CA, KB, CB)                                                        \
    {                                                                               \
        const lmask sw = lanes(KB < KA);                                            \
        const float ka = sel(sw, KA, KB), kb = sel(sw, KB, KA);                     \
        const int32_t ca = sel(sw, CA, CB), cb = sel(sw, CB, CA);                   \
        KA = ka, KB = kb, CA = ca, CB = cb;                                         \
    }
    RT_CE(k0, c0, k1, c1)
    RT_CE(k2, c2, k3, c3)
    RT_CE(k0, c0, k2, c2)
    RT_CE(k1, c1, k3, c3)
    RT_CE(k1, c1, k2, c2)
#undef RT_CE
    const bool descend = k0 < inf;
    if (lanes(!stack_shallow(stack, T, 3u)) == 0ull) { // every lane of this step: LDS only
        *lds_at(T.sp) = c3; // farthest first; the word is written in any case, only the stack pointer depends on the key
        T.sp = sel(lanes(k3 < inf), T.sp, T.sp + stack.pitch);
        *lds_at(T.sp) = c2;
        T.sp = sel(lanes(k2 < inf), T.sp, T.sp + stack.pitch);
        *lds_at(T.sp) = c1;
        T.sp = sel(lanes(k1 < inf), T.sp, T.sp + stack.pitch);
        if (descend) T.cur = c0;
        else trav_pop_lds(T, stack);
    } else {
        if (k3 < inf) stk_push(stack, T, c3);
        if (k2 < inf) stk_push(stack, T, c2);
        if (k1 < inf) stk_push(stack, T, c1);
        if (descend) T.cur = c0;
        else trav_pop(T, stack);
    }
}

} // namespace rt
