// rt_path_query.hip — path queries: radiance along caller-supplied rays, rt_trace_paths[_device] and their kernel k_path_query.
// (A unit of its own, as rt_query.hip and rt_gbuffer.hip are: a further traversal kernel inside an existing unit changes that unit's
// listings. tests/test_path_query.py runs the ISA hazard scan of tests/test_isa_hazards.py on this unit's listing.)
#include "rt_internal.h"
#include "rt_bounce.h"

namespace rt {

// k_megakernel's launch shape and round constants (rt_launch.h, rt_kernels.h): the kernel runs the same traversal steps and the same shading
// round under the same register budget
constexpr uint32_t kPathBlock = kMegaBlock, kPathWaves = kMegaWaves;
constexpr int kPathUnroll = 3;          // traversal steps between two checks of the loop's exit condition (kMegaUnroll)
#ifndef RT_PATH_SHADE_PCT
#define RT_PATH_SHADE_PCT 75
#endif
constexpr uint32_t kPathShadePct = RT_PATH_SHADE_PCT; // shade when this share of the live lanes is waiting (kMegaShadePct)
#ifndef RT_PATH_REFILL
#define RT_PATH_REFILL 16
#endif
constexpr uint32_t kPathRefill = RT_PATH_REFILL; // idle lanes after a shading round that make the wave take new rays (kQueryRefill)
// the ray cursors are the scene's, k_query's: 32 shards of the ray list with a cursor each on a 128-byte line, claimed 64 rays at a time
constexpr uint32_t kPathChunk = 64, kPathHeads = 32, kPathHeadStride = 16; // (stride in 8-byte words)
static_assert(kPathHeads * kPathHeadStride * 8u == kQueryCursorBytes, "the scene's cursor block holds one 128-byte line per shard");
static_assert(kPathRefill >= 1u && kPathRefill <= 64u, "a wave has 64 lanes");

// what a launch reads and writes (include/rt_mi355x.h: rt_path_query; NULL outputs are not written)
struct PathDev {
    const float* org;
    const float* dir;
    const uint32_t* rng;
    uint32_t* rng_out;
    float* radiance;
    uint32_t* rays;
    unsigned long long* cursor; // kPathHeads shard cursors, kPathHeadStride words apart; 0 at the launch (reset on its stream)
    uint32_t n, max_depth, samples, rr_start;
    ContractRange range; // rt_frame.hip: contract_range of the scene
};

// A path's first ray: get_ray without the camera and without its two draws (rt_device.h: camera_ray's RayData constructor)
RT_DEV RayState path_first_ray(const PathDev& q, uint32_t i, f3 o) {
    RayState r;
    r.org = o;
    r.dir[0] = f2h(q.dir[3 * (size_t)i]), r.dir[1] = f2h(q.dir[3 * (size_t)i + 1]), r.dir[2] = f2h(q.dir[3 * (size_t)i + 2]);
    r.att[0] = r.att[1] = r.att[2] = 0x3C00; // half(1.0)
    r.rad[0] = r.rad[1] = r.rad[2] = 0;      // half(0.0)
    return r;
}

// render_pixel's loops over a ray list instead of a pixel grid. k_query's persistent waves — a wave claims kPathChunk rays at a time from a
// shard cursor and hands them to its idle lanes — around k_megakernel's rounds: the lanes with a ray take whole-leaf traversal steps until
// kPathShadePct of them hold a finished traversal; those shade (shade_bounce with the staged tables, then the roulette) and either start the
// next bounce, restart from org[i] / dir[i] for the entry's next path, or store the entry's result and fall idle. After a round that leaves
// kPathRefill lanes idle the wave refills them all. Once every shard is exhausted the wave runs until its lanes are done and ends. No lane
// waits for another lane or another wave: the only barrier is the one of the LDS fill, before the loop.
// Per lane and through the traversal loop: the ray index, the RNG word, the path, bounce and ray counters and the ray's half state. The
// entry's colour sum is touched once per path, so it lives in LDS (three planes, one slot per lane), as k_megakernel's does: in registers it
// would be three more of the 80 through every traversal step. The ray count stays a register: as a fourth plane it took the workgroup from
// 53,696 to 55,744 bytes of LDS, past a third of the CU's 160 KB, and the kernel from 6 waves per SIMD to 4.
__global__ void __launch_bounds__(kPathBlock, kPathWaves) k_path_query(SceneDev S, PathDev q) {
    __shared__ float color_lds[3 * kPathBlock];
    typedef __attribute__((address_space(3))) float lds_f32;
    lds_f32* const color_r = (lds_f32*)color_lds + threadIdx.x;
    lds_f32* const color_g = color_r + kPathBlock;
    lds_f32* const color_b = color_g + kPathBlock;
    RayState r{};
    Trav T;
    RT_SHADE_LDS
    RT_TRAVERSAL_LDS(kPathBlock)
    T.cur = kTravDone;
    uint32_t ray = 0; // the lane's entry while `live`
    uint32_t rng = 0, s = 0, depth = 0, n_rays = 0;
    bool live = false;
    // wave-uniform: the shard drawn on, shards found exhausted, the claimed rays not yet handed out [cb, ce)
    uint32_t head = blockIdx.x % kPathHeads, heads_done = 0;
    uint32_t cb = 0, ce = 0;
    for (;;) {
        // REFILL every idle lane (or until every shard is exhausted) once kPathRefill lanes are idle; a wave without a live lane always does
        if (heads_done < kPathHeads || cb != ce) {
            const uint32_t n_idle = (uint32_t)__popcll(__ballot(!live));
            if (n_idle >= kPathRefill || n_idle == 64u) {
                for (;;) {
                    const lmask idle = __ballot(!live);
                    const uint32_t cnt = (uint32_t)__popcll(idle);
                    if (cnt == 0u) break;
                    while (cb == ce && heads_done < kPathHeads) { // claim: the next chunk of this shard, or move on to the next shard
                        const uint32_t lo = (uint32_t)((unsigned long long)q.n * head / kPathHeads);
                        const uint32_t len = (uint32_t)((unsigned long long)q.n * (head + 1u) / kPathHeads) - lo;
                        unsigned long long o = 0;
                        if ((threadIdx.x & 63u) == 0u) o = atomicAdd(q.cursor + head * kPathHeadStride, (unsigned long long)kPathChunk);
                        const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o < len ? o : len)); // (o < 2^32: n is 32 bits, every wave overshoots a shard once)
                        if (at < len) {
                            cb = lo + at, ce = lo + (len - at > kPathChunk ? at + kPathChunk : len);
                        } else {
                            head = head + 1u == kPathHeads ? 0u : head + 1u, heads_done++;
                        }
                    }
                    if (cb == ce) break; // every shard exhausted
                    const uint32_t take = ce - cb < cnt ? ce - cb : cnt;
                    const uint32_t rank = lane_rank(idle);
                    if (!live && rank < take) {
                        const uint32_t i = cb + rank; // < n: [cb, ce) lies inside its shard
                        const f3 o = mk3(q.org[3 * (size_t)i], q.org[3 * (size_t)i + 1], q.org[3 * (size_t)i + 2]);
                        const uint32_t a = q.rng[i];
                        if (in_contract_range(q.range, o.x, o.y, o.z)) {
                            r = path_first_ray(q, i, o);
                            rng = a, s = 0, depth = 0;
                            *color_r = 0.0f, *color_g = 0.0f, *color_b = 0.0f;
                            n_rays = 0u;
                            trav_begin(T, r.org, ray_dir(r), stack);
                            ray = i, live = true;
                        } else { // rejected: marked, never traced (the lane stays idle and takes the next ray)
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
        // TRAVERSE until kPathShadePct of the lanes that have a ray are waiting for shading
        const TravSigns sg = trav_signs(T); // every ray of this traversal phase has been started by now
        const uint32_t shade_at = n_live * kPathShadePct;
        for (;;) {
            if ((uint32_t)__popcll(__ballot(live && T.cur == kTravDone)) * 100u >= shade_at) break;
#pragma unroll
            for (int k = 0; k < kPathUnroll; ++k) (void)trav_step_wave<false, true>(S, T, stack, top, sg);
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
                if (s < q.samples) { // the entry's next path: the same first segment, the state the last path left
                    depth = 0;
                    r = path_first_ray(q, ray, mk3(q.org[3 * (size_t)ray], q.org[3 * (size_t)ray + 1], q.org[3 * (size_t)ray + 2]));
                } else { // entry finished
                    live = false;
                    const float n = (float)q.samples;
                    q.radiance[3 * (size_t)ray] = *color_r / n, q.radiance[3 * (size_t)ray + 1] = *color_g / n, q.radiance[3 * (size_t)ray + 2] = *color_b / n;
                    if (q.rng_out) q.rng_out[ray] = rng;
                    if (q.rays) q.rays[ray] = n_rays;
                }
            }
            if (live) trav_begin(T, r.org, ray_dir(r), stack);
        }
        __builtin_amdgcn_s_setprio(2);
    }
}

} // namespace rt

namespace {

int path_check(const rt_scene* s, const rt_path_query* q) {
    if (!s || !q) return fail(RT_ERR_INVALID, "null argument");
    if (q->max_depth == 0) return fail(RT_ERR_INVALID, "max_depth must be at least 1");
    if (q->samples == 0) return fail(RT_ERR_INVALID, "samples must be at least 1");
    if (q->n == 0) return RT_OK;
    if (!q->org || !q->dir) return fail(RT_ERR_INVALID, "null org or dir");
    if (!q->rng) return fail(RT_ERR_INVALID, "null rng: every ray needs its xorshift32 state");
    if (!q->radiance) return fail(RT_ERR_INVALID, "null radiance output");
    if (s->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    return RT_OK;
}

// the cursor reset, the launch and the event rt_scene_update waits for (PRE: path_check passed, n > 0, pointers on the scene's device)
int path_enqueue(rt_scene* s, const rt_path_query* q, hipStream_t st) {
    HIPCHK(hipSetDevice(s->device));
    if (!s->path_grid) { // persistent: as many workgroups as are resident at once
        int cus = 0, per_cu = 0;
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_path_query, (int)kPathBlock, 0));
        s->path_grid = (uint32_t)std::max(1, cus * std::max(1, per_cu));
        if (const char* e = dev_knob("RT_PATH_GRID")) s->path_grid = (uint32_t)std::max(1, std::atoi(e)); // tests: a grid far below the ray list's, so every wave refills mid-flight
    }
    hipEvent_t ev = nullptr;
    if (const int rc = scene_stream_event(s, st, &ev)) return rc;
    if (s->query_launched && s->query_stream != st) { // the cursors are the scene's, shared with the ray queries: the last launch that used them, on another stream, ends first
        hipEvent_t prev = nullptr;
        if (const int rc = scene_stream_event(s, s->query_stream, &prev)) return rc;
        HIPCHK(hipStreamWaitEvent(st, prev, 0));
    }
    PathDev d;
    d.org = q->org, d.dir = q->dir, d.rng = q->rng, d.rng_out = q->rng_out, d.radiance = q->radiance, d.rays = q->rays;
    d.cursor = s->d_query_cursor;
    d.n = q->n, d.max_depth = q->max_depth, d.samples = q->samples, d.rr_start = q->rr_start;
    d.range = contract_range(s->hs);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(s->path_grid, ((uint64_t)q->n + kPathBlock - 1u) / kPathBlock);
    HIPCHK(hipMemsetAsync(s->d_query_cursor, 0, kQueryCursorBytes, st));
    hipLaunchKernelGGL(k_path_query, dim3(grid), dim3(kPathBlock), 0, st, s->dev, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev, st));
    s->query_stream = st, s->query_launched = true;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_trace_paths(rt_scene* s, const rt_path_query* q) {
    if (const int rc = path_check(s, q)) return rc;
    const uint32_t n = q->n;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < n; ++i) {
        const float* o = q->org + 3 * (size_t)i;
        if (!in_contract_range(range, o[0], o[1], o[2]))
            return fail(RT_ERR_INVALID, "ray " + std::to_string(i) + ": origin more than 100 scene scales outside the scene's bounds or not finite (outside the range of the closest-hit contract)");
    }
    HIPCHK(hipSetDevice(s->device));
    DevBuf b_org, b_dir, b_rng, b_rad, b_rays;
    HIPCHK(b_org.alloc((size_t)n * 12));
    HIPCHK(b_dir.alloc((size_t)n * 12));
    HIPCHK(b_rng.alloc((size_t)n * 4));
    HIPCHK(b_rad.alloc((size_t)n * 12));
    HIPCHK(hipMemcpy(b_org.p, q->org, (size_t)n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_dir.p, q->dir, (size_t)n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_rng.p, q->rng, (size_t)n * 4, hipMemcpyHostToDevice));
    rt_path_query d = *q;
    d.org = b_org.as<float>(), d.dir = b_dir.as<float>(), d.rng = b_rng.as<uint32_t>(), d.radiance = b_rad.as<float>();
    d.rng_out = q->rng_out ? b_rng.as<uint32_t>() : nullptr; // in place on the device
    if (q->rays) HIPCHK(b_rays.alloc((size_t)n * 4));
    d.rays = b_rays.as<uint32_t>();
    if (const int rc = path_enqueue(s, &d, 0)) return rc;
    HIPCHK(hipStreamSynchronize(0));
    HIPCHK(hipMemcpy(q->radiance, b_rad.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    if (q->rng_out) HIPCHK(hipMemcpy(q->rng_out, b_rng.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (q->rays) HIPCHK(hipMemcpy(q->rays, b_rays.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_trace_paths_device(rt_scene* s, const rt_path_query* q, void* stream) {
    if (const int rc = path_check(s, q)) return rc;
    if (q->n == 0) return RT_OK;
    return path_enqueue(s, q, (hipStream_t)stream);
}

} // extern "C"
