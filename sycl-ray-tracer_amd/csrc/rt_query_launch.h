// rt_query_launch.h — the host half the query units share (rt_query.hip, rt_closest.hip, rt_multihit.hip, rt_nearest.hip, rt_path_query.hip,
// rt_path_gather.hip): the sizing of a query kernel's persistent grid, the launch on the scene's shared cursors (rt_scene_update relies on
// its event), the staging of a host form (query_staged) and the refusals two kinds word alike; what the two k-list kinds have in common
// beyond that: the choice of the list size with its grid, and the slot-major outputs; and what path and gather queries have: the argument
// checks.
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
    d.cursor = s->d_query_cursor.get();
    d.range = contract_range(s->hs);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(s->query_grid[kind], (n + block - 1u) / block);
    HIPCHK(hipMemsetAsync(s->d_query_cursor.get(), 0, kQueryCursorBytes, st));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, s->dev, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev, st));
    s->query_stream = st, s->query_launched = true;
    return RT_OK;
}

// The host form of a query: the caller's arrays are staged on the scene's device around one launch on the null stream. A buffer holds
// `bytes` per entry; host == NULL: not allocated and not copied, so the launch sees its NULL. An output with in_place >= 0 has no buffer
// of its own: the kernel writes it into that input's (the path kinds' rng -> rng_out; only the list says so). In order: hipSetDevice,
// the allocations, the copies in, enqueue(in, out) with the device pointers by list index, hipStreamSynchronize(0), the copies out. PRE: checks passed, n > 0.
struct StageIn { const void* host; size_t bytes; };
struct StageOut { void* host; size_t bytes; int in_place = -1; };
template <size_t NI, size_t NO, class Enqueue>
int query_staged(rt_scene* s, size_t n, const StageIn (&ins)[NI], const StageOut (&outs)[NO], Enqueue enqueue) {
    HIPCHK(hipSetDevice(s->device));
    DevBuf b_in[NI], b_out[NO];
    void *in[NI], *out[NO];
    for (size_t k = 0; k < NI; ++k) {
        if (ins[k].host) HIPCHK(b_in[k].alloc(n * ins[k].bytes));
        in[k] = b_in[k].p;
    }
    for (size_t k = 0; k < NO; ++k) {
        if (outs[k].host && outs[k].in_place < 0) HIPCHK(b_out[k].alloc(n * outs[k].bytes));
        out[k] = outs[k].host && outs[k].in_place >= 0 ? in[outs[k].in_place] : b_out[k].p;
    }
    for (size_t k = 0; k < NI; ++k)
        if (ins[k].host) HIPCHK(hipMemcpy(in[k], ins[k].host, n * ins[k].bytes, hipMemcpyHostToDevice));
    if (const int rc = enqueue(in, out)) return rc;
    HIPCHK(hipStreamSynchronize(0));
    for (size_t k = 0; k < NO; ++k)
        if (outs[k].host) HIPCHK(hipMemcpy(outs[k].host, out[k], n * outs[k].bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- the k-list kinds (rt_multihit.hip, rt_nearest.hip; the list: rt_hit_list.h) -------------------------------------------------------------
// One instantiation per list size, N = 2, 4 or 8 slots, the smallest that holds d.k, each with a persistent grid of its own (base + 0, + 1,
// + 2), sized for its own occupancy at the scene's first launch of it: what a call takes does not depend on the k of the calls before it.
// kernel_of(ListSize<N>{}) -> the unit's kernel of N slots; grid_knob as query_launch's.
template <uint32_t N> using ListSize = std::integral_constant<uint32_t, N>;
template <QueryKind Base, class Dev, class KernelOf>
int list_launch(rt_scene* s, KernelOf kernel_of, uint32_t block, const Dev& d, hipStream_t st, const char* grid_knob) {
    const auto go = [&](auto n) {
        constexpr uint32_t N = decltype(n)::value;
        constexpr QueryKind kind = (QueryKind)(Base + (N == 2 ? 0 : N == 4 ? 1 : 2));
        static_assert((N == 2 || N == 4 || N == 8) && kind < kQueryKinds, "three instantiations, three grids");
        return query_launch(s, kind, kernel_of(n), block, d, d.n, st, grid_knob);
    };
    return d.k <= 2 ? go(ListSize<2>{}) : d.k <= 4 ? go(ListSize<4>{}) : go(ListSize<8>{});
}
// the outputs of a k-list query's host form: four slot-major arrays of k slots per entry, and the count
inline void list_stage_outs(StageOut (&outs)[5], uint32_t k, float* t, float* u, float* v, uint32_t* tri, uint32_t* count) {
    const size_t slot = 4 * (size_t)k; // bytes per entry of a slot-major output
    outs[0] = {t, slot}, outs[1] = {u, slot}, outs[2] = {v, slot}, outs[3] = {tri, slot}, outs[4] = {count, 4};
}

// the refusals with one wording in every kind
inline int refuse_host_only(const rt_scene* s) { return s->device < 0 ? fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)") : RT_OK; }
inline int refuse_ray_origin(const ContractRange& range, const float* org, uint32_t i) {
    const float* o = org + 3 * (size_t)i;
    if (!in_contract_range(range, o[0], o[1], o[2]))
        return fail(RT_ERR_INVALID, "ray " + std::to_string(i) + ": origin more than 100 scene scales outside the scene's bounds or not finite (outside the range of the closest-hit contract)");
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
    return refuse_host_only(s);
}

// the device form: check, enqueue
inline int paths_device(rt_scene* s, const PathArgs& a, const PathKind& k, hipStream_t st) {
    if (const int rc = path_args_check(s, a, k)) return rc;
    return a.n == 0 ? RT_OK : k.enqueue(s, a, st);
}

// the host form: check, refuse per entry, stage (query_staged)
inline int paths_host(rt_scene* s, const PathArgs& a, const PathKind& k) {
    if (const int rc = path_args_check(s, a, k)) return rc;
    const size_t n = a.n;
    if (n == 0) return RT_OK;
    const ContractRange range = contract_range(s->hs);
    for (uint32_t i = 0; i < a.n; ++i)
        if (const int rc = k.refuse(range, a, i)) return rc;
    const StageIn ins[3] = {{a.in0, 12}, {a.in1, 12}, {a.rng, 4}};
    const StageOut outs[3] = {{a.radiance, 12}, {a.rng_out, 4, 2}, {a.rays, 4}}; // rng_out: in place on the device, in rng's buffer
    return query_staged(s, n, ins, outs, [&](void* const* in, void* const* out) {
        PathArgs d = a;
        d.in0 = (const float*)in[0], d.in1 = (const float*)in[1], d.rng = (const uint32_t*)in[2];
        d.radiance = (float*)out[0], d.rng_out = (uint32_t*)out[1], d.rays = (uint32_t*)out[2];
        return k.enqueue(s, d, 0);
    });
}

} // namespace rtlib
