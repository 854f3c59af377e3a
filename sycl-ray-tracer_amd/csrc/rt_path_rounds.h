// rt_path_rounds.h — the body k_path_query (rt_path_query.hip) and k_path_gather (rt_path_gather.hip) share: persistent waves around
// k_megakernel's traversal and shading rounds, over a list of entries instead of a pixel grid. Each of the two units keeps its launch struct, a
// policy struct E and a one-line __global__ wrapper (the claim of entries and their hand-out to idle lanes is rt_query_frame.h's, shared
// with the other query kernels); what differs between them is in E alone:
//   E::load(q, i)         the floats of entry i, in a type of E's choosing that only E's other functions look into
//   E::ok(q, e)           whether the entry is traced (a rejected one is marked, never traced, and its lane takes the next entry)
//   E::first(q, i, e, a)  the first ray of the entry's first path, from the floats just loaded; `a` is the entry's RNG word, advanced by what is drawn
//   E::next(q, i, rng)    the first ray of each further path, the entry's floats re-read from memory (one L2 read per path, instead of
//                         riding in registers through the traversal loop)
//   E::kBlock, kRefill, kShadePct, kUnroll   the launch shape and round constants
// Every function RETURNS its value, and path_rounds takes the scene and the launch struct BY VALUE: a RayState out-parameter, or references to
// the two structs, cost k_path_query three more spilled registers (EXPERIMENTS.md).
#pragma once
#include "rt_internal.h"
#include "rt_bounce.h"
#include "rt_query_frame.h"

namespace rt {

// render_pixel's loops over an entry list. The query kernels' persistent waves — a wave claims kQueryChunk entries at a time from a shard cursor and
// hands them to its idle lanes — around k_megakernel's rounds: the lanes with a ray take whole-leaf traversal steps until E::kShadePct of
// them hold a finished traversal; those shade (shade_bounce with the staged tables, then the roulette) and either start the next bounce,
// restart with E::next for the entry's next path, or store the entry's result and fall idle. After a round that leaves E::kRefill lanes
// idle the wave refills them all. Once every shard is exhausted the wave runs until its lanes are done and ends. An entry is one lane's
// sequential work: no lane waits for another lane or another wave, there is no cross-lane reduction and no atomic on a result; the only
// barrier is the one of the LDS fill, before the loop.
// Per lane and through the traversal loop: the entry's index, the RNG word, the path, bounce and ray counters and the ray's half state. The
// entry's colour sum is touched once per path, so it lives in LDS (three planes, one slot per lane), as k_megakernel's does: in registers it
// would be three more of the 80 through every traversal step. The ray count stays a register: as a fourth plane it took the workgroup from
// 53,696 to 55,744 bytes of LDS, past a third of the CU's 160 KB, and the kernel from 6 waves per SIMD to 4.
template <class E, class Q>
RT_DEV void path_rounds(SceneDev S, Q q) {
    __shared__ float color_lds[3 * E::kBlock];
    typedef __attribute__((address_space(3))) float lds_f32;
    lds_f32* const color_r = (lds_f32*)color_lds + threadIdx.x;
    lds_f32* const color_g = color_r + E::kBlock;
    lds_f32* const color_b = color_g + E::kBlock;
    RayState r{};
    Trav T;
    RT_SHADE_LDS
    RT_TRAVERSAL_LDS(E::kBlock)
    T.cur = kTravDone;
    uint32_t ent = 0; // the lane's entry while `live`
    uint32_t rng = 0, s = 0, depth = 0, n_rays = 0;
    bool live = false;
    Claim claim = claim_begin(); // wave-uniform (rt_query_frame.h)
    for (;;) {
        // REFILL every idle lane (or until every shard is exhausted) once E::kRefill lanes are idle; a wave without a live lane always does
        if (claim_open(claim)) {
            const uint32_t n_idle = (uint32_t)__popcll(__ballot(!live));
            if (n_idle >= E::kRefill || n_idle == 64u) {
                claim = claim_refill(claim, ClaimList{q.cursor, q.n}, [&] { return !live; }, [&](uint32_t i) {
                    const auto e = E::load(q, i);
                    uint32_t a = q.rng[i];
                    if (E::ok(q, e)) {
                        r = E::first(q, i, e, a);
                        rng = a, s = 0, depth = 0;
                        *color_r = 0.0f, *color_g = 0.0f, *color_b = 0.0f;
                        n_rays = 0u;
                        trav_begin(T, r.org, ray_dir(r), stack);
                        ent = i, live = true;
                    } else { // rejected: marked, never traced, no draw taken (the lane stays idle and takes the next entry)
                        const float nan = __builtin_nanf("");
                        q.radiance[3 * (size_t)i] = nan, q.radiance[3 * (size_t)i + 1] = nan, q.radiance[3 * (size_t)i + 2] = nan;
                        if (q.rays) q.rays[i] = 0xFFFFFFFFu;
                        if (q.rng_out) q.rng_out[i] = a;
                    }
                });
            }
        }
        const uint32_t n_live = (uint32_t)__popcll(__ballot(live));
        if (n_live == 0u) break; // (no lane is live after a refill only when every shard is exhausted)
        // TRAVERSE until E::kShadePct of the lanes that have a ray are waiting for shading
        const TravSigns sg = trav_signs(T); // every ray of this traversal phase has been started by now
        const uint32_t shade_at = n_live * E::kShadePct;
        const lmask live_m = lanes(live);
        for (;;) {
            const lmask done = trav_done(T);
            if (count(done & live_m) * 100u >= shade_at) break;
            (void)trav_step_wave<false, true>(S, T, stack, top, sg, trav_classes(T, done));
#pragma unroll
            for (int k = 1; k < E::kUnroll; ++k) (void)trav_step_wave<false, true>(S, T, stack, top, sg);
        }
        // SHADE the lanes whose traversal is complete
        __builtin_amdgcn_s_setprio(0);
        if (live && T.cur == kTravDone) {
            n_rays++;
            f3 res;
            const bool done = shade_bounce<true>(S, rng, r, T.best, res, &T, &tab);
            if (done) *color_r = *color_r + res.x, *color_g = *color_g + res.y, *color_b = *color_b + res.z; // (a path that is killed or outlives max_depth adds nothing)
            depth++;
            bool killed = false;
            if (q.rr_start && !done && depth >= q.rr_start && depth < q.max_depth) killed = !roulette(rng, r);
            if (done || killed || depth == q.max_depth) {
                s++;
                if (s < q.samples) { // the entry's next path, from the state the last path left
                    depth = 0;
                    r = E::next(q, ent, rng);
                } else { // entry finished
                    live = false;
                    const float n = (float)q.samples;
                    q.radiance[3 * (size_t)ent] = *color_r / n, q.radiance[3 * (size_t)ent + 1] = *color_g / n, q.radiance[3 * (size_t)ent + 2] = *color_b / n;
                    if (q.rng_out) q.rng_out[ent] = rng;
                    if (q.rays) q.rays[ent] = n_rays;
                }
            }
            if (live) trav_begin(T, r.org, ray_dir(r), stack);
        }
        __builtin_amdgcn_s_setprio(2);
    }
}

} // namespace rt
