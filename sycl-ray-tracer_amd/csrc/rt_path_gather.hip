// rt_path_gather.hip — gather queries: diffuse-lobe radiance at caller-supplied points, rt_gather_paths[_device] and their kernel k_path_gather.
// (A unit of its own, as rt_path_query.hip is: a further traversal kernel inside an existing unit changes that unit's listings.
// tests/test_gather.py runs the ISA hazard scan of tests/test_isa_hazards.py on this unit's listing.)
#include "rt_internal.h"
#include "rt_bounce.h"

namespace rt {

// k_path_query's launch shape, round constants and cursors (rt_path_query.hip): the kernel is that one with another first ray
constexpr uint32_t kGatherBlock = kMegaBlock, kGatherWaves = kMegaWaves;
constexpr int kGatherUnroll = 3;          // traversal steps between two checks of the loop's exit condition (kMegaUnroll)
#ifndef RT_GATHER_SHADE_PCT
#define RT_GATHER_SHADE_PCT 75
#endif
constexpr uint32_t kGatherShadePct = RT_GATHER_SHADE_PCT; // shade when this share of the live lanes is waiting (kMegaShadePct)
#ifndef RT_GATHER_REFILL
#define RT_GATHER_REFILL 16
#endif
constexpr uint32_t kGatherRefill = RT_GATHER_REFILL; // idle lanes after a shading round that make the wave take new entries (kQueryRefill)
// the cursors are the scene's, k_query's: 32 shards of the entry list with a cursor each on a 128-byte line, claimed 64 entries at a time
constexpr uint32_t kGatherChunk = 64, kGatherHeads = 32, kGatherHeadStride = 16; // (stride in 8-byte words)
static_assert(kGatherHeads * kGatherHeadStride * 8u == kQueryCursorBytes, "the scene's cursor block holds one 128-byte line per shard");
static_assert(kGatherRefill >= 1u && kGatherRefill <= 64u, "a wave has 64 lanes");

// what a launch reads and writes (include/rt_mi355x.h: rt_gather_query; NULL outputs are not written)
struct GatherDev {
    const float* pos;
    const float* normal;
    const uint32_t* rng;
    uint32_t* rng_out;
    float* radiance;
    uint32_t* rays;
    unsigned long long* cursor; // kGatherHeads shard cursors, kGatherHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n, max_depth, samples, rr_start;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

RT_DEV f3 gather_load3(const float* p, uint32_t i) { return mk3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }

// A path's first ray: the diffuse bounce's own scattered ray (rt_device.h: scatter, normal + rng_unit_vector, without the near_zero clause,
// which tests an incoming direction that does not exist here) from pos[i], with the attenuation and radiance of a camera ray. Three draws.
RT_DEV RayState gather_first_ray(uint32_t& rng, f3 o, f3 nrm) {
    RayState r;
    const f3 d = nrm + rng_unit_vector(rng);
    r.org = o;
    r.dir[0] = f2h(d.x), r.dir[1] = f2h(d.y), r.dir[2] = f2h(d.z);
    r.att[0] = r.att[1] = r.att[2] = 0x3C00; // half(1.0)
    r.rad[0] = r.rad[1] = r.rad[2] = 0;      // half(0.0)
    return r;
}

// k_path_query (rt_path_query.hip) with one difference: where that kernel builds a path's first ray from org[i] / dir[i], this one builds it
// from pos[i], normal[i] and three draws on the entry's running state, at the refill and at every restart for the entry's next path (the
// entry's six floats are re-read from memory there, one L2 read per path, instead of riding in registers through the traversal loop).
// Persistent waves claim kGatherChunk entries at a time from a shard cursor and hand them to their idle lanes; the lanes with a ray take
// whole-leaf traversal steps until kGatherShadePct of them hold a finished traversal; those shade, run the roulette and either start the next
// bounce, restart, or store the entry's mean and fall idle. An entry is one lane's sequential work: no lane waits for another lane or another
// wave, there is no cross-lane reduction and no atomic on a result; the only barrier is the one of the LDS fill, before the loop.
// The colour sum lives in LDS (three planes, one slot per lane) and the ray count in a register, for the reasons k_path_query states.
// (The claim / refill loop is k_path_query's text a third time: see DESIGN.md §18 on why it was not lifted into a header.)
__global__ void __launch_bounds__(kGatherBlock, kGatherWaves) k_path_gather(SceneDev S, GatherDev q) {
    __shared__ float color_lds[3 * kGatherBlock];
    typedef __attribute__((address_space(3))) float lds_f32;
    lds_f32* const color_r = (lds_f32*)color_lds + threadIdx.x;
    lds_f32* const color_g = color_r + kGatherBlock;
    lds_f32* const color_b = color_g + kGatherBlock;
    RayState r{};
    Trav T;
    RT_SHADE_LDS
    RT_TRAVERSAL_LDS(kGatherBlock)
    T.cur = kTravDone;
    uint32_t ent = 0; // the lane's entry while `live`
    uint32_t rng = 0, s = 0, depth = 0, n_rays = 0;
    bool live = false;
    // wave-uniform: the shard drawn on, shards found exhausted, the claimed entries not yet handed out [cb, ce)
    uint32_t head = blockIdx.x % kGatherHeads, heads_done = 0;
    uint32_t cb = 0, ce = 0;
    for (;;) {
        // REFILL every idle lane (or until every shard is exhausted) once kGatherRefill lanes are idle; a wave without a live lane always does
        if (heads_done < kGatherHeads || cb != ce) {
            const uint32_t n_idle = (uint32_t)__popcll(__ballot(!live));
            if (n_idle >= kGatherRefill || n_idle == 64u) {
                for (;;) {
                    const lmask idle = __ballot(!live);
                    const uint32_t cnt = (uint32_t)__popcll(idle);
                    if (cnt == 0u) break;
                    while (cb == ce && heads_done < kGatherHeads) { // claim: the next chunk of this shard, or move on to the next shard
                        const uint32_t lo = (uint32_t)((unsigned long long)q.n * head / kGatherHeads);
                        const uint32_t len = (uint32_t)((unsigned long long)q.n * (head + 1u) / kGatherHeads) - lo;
                        unsigned long long o = 0;
                        if ((threadIdx.x & 63u) == 0u) o = atomicAdd(q.cursor + head * kGatherHeadStride, (unsigned long long)kGatherChunk);
                        const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o < len ? o : len)); // (o < 2^32: n is 32 bits, every wave overshoots a shard once)
                        if (at < len) {
                            cb = lo + at, ce = lo + (len - at > kGatherChunk ? at + kGatherChunk : len);
                        } else {
                            head = head + 1u == kGatherHeads ? 0u : head + 1u, heads_done++;
                        }
                    }
                    if (cb == ce) break; // every shard exhausted
                    const uint32_t take = ce - cb < cnt ? ce - cb : cnt;
                    const uint32_t rank = lane_rank(idle);
                    if (!live && rank < take) {
                        const uint32_t i = cb + rank; // < n: [cb, ce) lies inside its shard
                        const f3 o = gather_load3(q.pos, i);
                        const f3 nrm = gather_load3(q.normal, i);
                        uint32_t a = q.rng[i];
                        if (in_contract_range(q.range, o.x, o.y, o.z) && __builtin_isfinite(nrm.x) && __builtin_isfinite(nrm.y) && __builtin_isfinite(nrm.z)) {
                            r = gather_first_ray(a, o, nrm);
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
                    }
                    cb += take;
                }
            }
        }
        const uint32_t n_live = (uint32_t)__popcll(__ballot(live));
        if (n_live == 0u) break; // (no lane is live after a refill only when every shard is exhausted)
        // TRAVERSE until kGatherShadePct of the lanes that have a ray are waiting for shading
        const TravSigns sg = trav_signs(T); // every ray of this traversal phase has been started by now
        const uint32_t shade_at = n_live * kGatherShadePct;
        for (;;) {
            if ((uint32_t)__popcll(__ballot(live && T.cur == kTravDone)) * 100u >= shade_at) break;
#pragma unroll
            for (int k = 0; k < kGatherUnroll; ++k) (void)trav_step_wave<false, true>(S, T, stack, top, sg);
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
                if (s < q.samples) { // the entry's next path: a direction of its own, drawn from the state the last path left
                    depth = 0;
                    r = gather_first_ray(rng, gather_load3(q.pos, ent), gather_load3(q.normal, ent));
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

namespace {

bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

int gather_check(const rt_scene* s, const rt_gather_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->max_depth == 0) return fail(RT_ERR_INVALID, "max_depth must be at least 1");
    if (q->samples == 0) return fail(RT_ERR_INVALID, "samples must be at least 1");
    if (q->n == 0) return RT_OK;
    if (!q->pos || !q->normal) return fail(RT_ERR_INVALID, "null pos or normal");
    if (!q->rng) return fail(RT_ERR_INVALID, "null rng: every entry needs its xorshift32 state");
    if (!q->radiance) return fail(RT_ERR_INVALID, "null radiance output");
    if (s->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    return RT_OK;
}

// the cursor reset, the launch and the event rt_scene_update waits for (PRE: gather_check passed, n > 0, pointers on the scene's device)
int gather_enqueue(rt_scene* s, const rt_gather_query* q, hipStream_t st) {
    HIPCHK(hipSetDevice(s->device));
    if (!s->gather_grid) { // persistent: as many workgroups as are resident at once
        int cus = 0, per_cu = 0;
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_path_gather, (int)kGatherBlock, 0));
        s->gather_grid = (uint32_t)std::max(1, cus * std::max(1, per_cu));
        if (const char* e = dev_knob("RT_GATHER_GRID")) s->gather_grid = (uint32_t)std::max(1, std::atoi(e)); // tests: a grid far below the entry list's, so every wave refills mid-flight
    }
    hipEvent_t ev = nullptr;
    if (const int rc = scene_stream_event(s, st, &ev)) return rc;
    if (s->query_launched && s->query_stream != st) { // the cursors are the scene's, shared with the ray and path queries: the last launch that used them, on another stream, ends first
        hipEvent_t prev = nullptr;
        if (const int rc = scene_stream_event(s, s->query_stream, &prev)) return rc;
        HIPCHK(hipStreamWaitEvent(st, prev, 0));
    }
    GatherDev d;
    d.pos = q->pos, d.normal = q->normal, d.rng = q->rng, d.rng_out = q->rng_out, d.radiance = q->radiance, d.rays = q->rays;
    d.cursor = s->d_query_cursor;
    d.n = q->n, d.max_depth = q->max_depth, d.samples = q->samples, d.rr_start = q->rr_start;
    d.range = contract_range(s->hs);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(s->gather_grid, ((uint64_t)q->n + kGatherBlock - 1u) / kGatherBlock);
    HIPCHK(hipMemsetAsync(s->d_query_cursor, 0, kQueryCursorBytes, st));
    hipLaunchKernelGGL(k_path_gather, dim3(grid), dim3(kGatherBlock), 0, st, s->dev, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev, st));
    s->query_stream = st, s->query_launched = true;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_gather_paths(rt_scene* s, const rt_gather_query* q) {
    if (const int rc = gather_check(s, q)) return rc;
    const uint32_t n = q->n;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < n; ++i) {
        const float* o = q->pos + 3 * (size_t)i;
        if (!in_contract_range(range, o[0], o[1], o[2]))
            return fail(RT_ERR_INVALID, "entry " + std::to_string(i) + ": position more than 100 scene scales outside the scene's bounds or not finite (outside the range of the closest-hit contract)");
        if (!finite3(q->normal + 3 * (size_t)i)) return fail(RT_ERR_INVALID, "entry " + std::to_string(i) + ": normal not finite");
    }
    HIPCHK(hipSetDevice(s->device));
    DevBuf b_pos, b_nrm, b_rng, b_rad, b_rays;
    HIPCHK(b_pos.alloc((size_t)n * 12));
    HIPCHK(b_nrm.alloc((size_t)n * 12));
    HIPCHK(b_rng.alloc((size_t)n * 4));
    HIPCHK(b_rad.alloc((size_t)n * 12));
    HIPCHK(hipMemcpy(b_pos.p, q->pos, (size_t)n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_nrm.p, q->normal, (size_t)n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_rng.p, q->rng, (size_t)n * 4, hipMemcpyHostToDevice));
    rt_gather_query d = *q;
    d.pos = b_pos.as<float>(), d.normal = b_nrm.as<float>(), d.rng = b_rng.as<uint32_t>(), d.radiance = b_rad.as<float>();
    d.rng_out = q->rng_out ? b_rng.as<uint32_t>() : nullptr; // in place on the device
    if (q->rays) HIPCHK(b_rays.alloc((size_t)n * 4));
    d.rays = b_rays.as<uint32_t>();
    if (const int rc = gather_enqueue(s, &d, 0)) return rc;
    HIPCHK(hipStreamSynchronize(0));
    HIPCHK(hipMemcpy(q->radiance, b_rad.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    if (q->rng_out) HIPCHK(hipMemcpy(q->rng_out, b_rng.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (q->rays) HIPCHK(hipMemcpy(q->rays, b_rays.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_gather_paths_device(rt_scene* s, const rt_gather_query* q, void* stream) {
    if (const int rc = gather_check(s, q)) return rc;
    if (q->n == 0) return RT_OK;
    return gather_enqueue(s, q, (hipStream_t)stream);
}

} // extern "C"
