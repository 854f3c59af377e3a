// rt_query_launch.h — the host half rt_query.hip, rt_path_query.hip and rt_path_gather.hip share: the sizing of a query kernel's persistent
// grid, the launch on the scene's shared cursors (rt_scene_update relies on its event), and what path and gather queries have in common
// beyond that: the argument checks and the staging of the host form.
#pragma once
#include "rt_internal.h"

namespace rtlib {

// The cursor reset, the launch of `kernel` over n entries and the event rt_scene_update waits for. PRE: the query's check passed, n > 0, d's
// pointers are on the scene's device. d.cursor and d.range are filled here. The grid is persistent: min(ceil(n / block), the workgroups of
// this kernel resident at once), the latter sized at the scene's first launch of `kind` — or set to grid_knob (a developer knob's value, for
// tests that want a grid far below the entry list's, so every wave refills mid-flight; read only at that first launch).
template <class Dev>
int query_launch(rt_scene* s, QueryKind kind, void (*kernel)(SceneDev, Dev), uint32_t block, Dev d, uint64_t n, hipStream_t st, const char* grid_knob = nullptr) {
    HIPCHK(hipSetDevice(s->device));
    if (!s->query_grid[kind]) {
        int cus = 0, per_cu = 0;
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)block, 0));
        s->query_grid[kind] = (uint32_t)std::max(1, cus * std::max(1, per_cu));
        if (grid_knob) s->query_grid[kind] = (uint32_t)std::max(1, std::atoi(grid_knob));
    }
    hipEvent_t ev = nullptr;
    if (const int rc = scene_stream_event(s, st, &ev)) return rc;
    if (s->query_launched && s->query_stream != st) { // the cursors are the scene's, shared by every query kind: the last launch that used them, on another stream, ends first
        hipEvent_t prev = nullptr;
        if (const int rc = scene_stream_event(s, s->query_stream, &prev)) return rc;
        HIPCHK(hipStreamWaitEvent(st, prev, 0));
    }
    d.cursor = s->d_query_cursor;
    d.range = contract_range(s->hs);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(s->query_grid[kind], (n + block - 1u) / block);
    HIPCHK(hipMemsetAsync(s->d_query_cursor, 0, kQueryCursorBytes, st));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, s->dev, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev, st));
    s->query_stream = st, s->query_launched = true;
    return RT_OK;
}

// A path or a gather query by role (include/rt_mi355x.h: rt_path_query, rt_gather_query): in0 / in1 are org / dir or pos / normal.
struct PathArgs {
    uint32_t n, max_depth, samples, rr_start;
    const float* in0;
    const float* in1;
    const uint32_t* rng;
    uint32_t* rng_out;
    float* radiance;
    uint32_t* rays;
};
// ... and what a kind adds: its words for the messages, the host form's per-entry refusal (RT_OK, or fail() with the kind's text) and its launch
struct PathKind {
    const char* inputs; // "org or dir"
    const char* entry;  // "ray"
    int (*refuse)(const ContractRange& range, const PathArgs& a, uint32_t i);
    int (*enqueue)(rt_scene* s, const PathArgs& a, hipStream_t st);
};

inline int path_args_check(const rt_scene* s, const PathArgs& a, const PathKind& k) {
    if (a.max_depth == 0) return fail(RT_ERR_INVALID, "max_depth must be at least 1");
    if (a.samples == 0) return fail(RT_ERR_INVALID, "samples must be at least 1");
    if (a.n == 0) return RT_OK;
    if (!a.in0 || !a.in1) return fail(RT_ERR_INVALID, std::string("null ") + k.inputs);
    if (!a.rng) return fail(RT_ERR_INVALID, std::string("null rng: every ") + k.entry + " needs its xorshift32 state");
    if (!a.radiance) return fail(RT_ERR_INVALID, "null radiance output");
    if (s->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    return RT_OK;
}

// the device form: check, enqueue
inline int paths_device(rt_scene* s, const PathArgs& a, const PathKind& k, hipStream_t st) {
    if (const int rc = path_args_check(s, a, k)) return rc;
    return a.n == 0 ? RT_OK : k.enqueue(s, a, st);
}

// the host form: check, refuse per entry, stage the inputs, run on the null stream, copy the outputs back
inline int paths_host(rt_scene* s, const PathArgs& a, const PathKind& k) {
    if (const int rc = path_args_check(s, a, k)) return rc;
    const size_t n = a.n;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < a.n; ++i)
        if (const int rc = k.refuse(range, a, i)) return rc;
    HIPCHK(hipSetDevice(s->device));
    DevBuf b_in0, b_in1, b_rng, b_rad, b_rays;
    HIPCHK(b_in0.alloc(n * 12));
    HIPCHK(b_in1.alloc(n * 12));
    HIPCHK(b_rng.alloc(n * 4));
    HIPCHK(b_rad.alloc(n * 12));
    HIPCHK(hipMemcpy(b_in0.p, a.in0, n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_in1.p, a.in1, n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b_rng.p, a.rng, n * 4, hipMemcpyHostToDevice));
    PathArgs d = a;
    d.in0 = b_in0.as<float>(), d.in1 = b_in1.as<float>(), d.rng = b_rng.as<uint32_t>(), d.radiance = b_rad.as<float>();
    d.rng_out = a.rng_out ? b_rng.as<uint32_t>() : nullptr; // in place on the device
    if (a.rays) HIPCHK(b_rays.alloc(n * 4));
    d.rays = b_rays.as<uint32_t>();
    if (const int rc = k.enqueue(s, d, 0)) return rc;
    HIPCHK(hipStreamSynchronize(0));
    HIPCHK(hipMemcpy(a.radiance, b_rad.p, n * 12, hipMemcpyDeviceToHost));
    if (a.rng_out) HIPCHK(hipMemcpy(a.rng_out, b_rng.p, n * 4, hipMemcpyDeviceToHost));
    if (a.rays) HIPCHK(hipMemcpy(a.rays, b_rays.p, n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

} // namespace rtlib
