// rt_update.hip — dynamic scenes: what rt_scene_create_ex keeps for RT_SCENE_UPDATABLE, rt_scene_update and its kernels, and the lazy
// refresh of the host copy. A unit of its own, so that the render kernels (rt_frame.hip) compile to the same code as without it.
//
// An update keeps the BVH's topology (child words, leaf codes, node order) and recomputes everything geometric in place, in two phases:
//   1. k_upd_transform: every triangle's world-space vertices, with the host builder's expression (scene_rules.h: world_coord, compiled
//      with -ffp-contract=off on either side), into the scratch array `wv`; in the same pass the scene's bounds as ordered keys that also
//      carry the first occurrence (the host's std::min / std::max keep the first of equal values: the sign of a zero bound depends on it)
//      and a non-finite flag. The host reads back 7 words and applies rt_scene_create's test. A refusal restores `wv` and stops here:
//      nothing else of the scene has been written.
//   2. k_upd_records rewrites v0 / e1 / e2 of every leaf record, k_upd_refit the nodes, one launch per height level (a node's children lie in
//      lower levels, so the kernel boundary is the only hand-off between workgroups: no atomics, no fences), k_upd_words / k_upd_normals the
//      shading records where the instance table's rows moved / where normals were given.
// Every write lands in a buffer that exists since rt_scene_create: no device pointer of SceneDev changes. The kernels call the rules the host
// builder and the host refit use (scene_rules.h); the device form of the arrays they rewrite is rt_scene_image.h's.
#include "rt_internal.h"
#include "rt_scene_image.h"
#include "scene_rules.h"

#include <algorithm>
#include <limits>

namespace rtlib {
namespace {

// ---- ordered bound keys ------------------------------------------------------------------------------------------------------------------
// high word: the float in an order-preserving encoding (-0 and +0 alike); low word: the vertex slot 3t + k (< 2^30), reversed for the
// maximum, so that of equal values the first in scene order wins, and the sign of the value (what tells -0 from +0)
__host__ __device__ inline uint32_t order_key(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    if (f == 0.0f) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long min_key(float f, uint32_t v) {
    return ((unsigned long long)order_key(f) << 32) | (unsigned long long)((v << 1) | (__float_as_uint(f) >> 31));
}
__device__ __forceinline__ unsigned long long max_key(float f, uint32_t v) {
    return ((unsigned long long)order_key(f) << 32) | (unsigned long long)(((~v & 0x3FFFFFFFu) << 1) | (__float_as_uint(f) >> 31));
}
inline float key_value(unsigned long long key) {
    const uint32_t k = (uint32_t)(key >> 32);
    uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    if (b == 0u && (key & 1ull)) b = 0x80000000u; // -0
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

constexpr uint32_t kRedWords = 8; // [0, 3) min keys, [3, 6) max keys, [6] non-finite flag, [7] the refit's failure flag

// Phase 1: world-space vertices + bounds + non-finite flag. One thread per triangle. WRITE = false: the bounds and the flag only, `wv` untouched
// (a scene that keeps its previous vertices tests an update before it writes anything: a refusal must leave both copies as they were).
template <bool WRITE = true>
__global__ void __launch_bounds__(256) k_upd_transform(uint32_t n_tris, const float* __restrict__ pos, const uint32_t* __restrict__ idx,
                                                        const uint32_t* __restrict__ tri_inst, const float* __restrict__ xf,
                                                        float* __restrict__ wv, unsigned long long* __restrict__ red) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    unsigned long long kmin[3] = {~0ull, ~0ull, ~0ull}, kmax[3] = {0ull, 0ull, 0ull};
    uint32_t bad = 0;
    if (t < n_tris) {
        const float* m = xf + 16 * (size_t)tri_inst[t];
        for (int k = 0; k < 3; ++k) {
            const uint32_t vi = idx[3 * (size_t)t + k];
            const float x = pos[3 * (size_t)vi], y = pos[3 * (size_t)vi + 1], z = pos[3 * (size_t)vi + 2];
            for (int a = 0; a < 3; ++a) {
                const float p = world_coord(m, a, x, y, z);
                if (WRITE) wv[9 * (size_t)t + 3 * k + a] = p;
                bad |= isfinite(p) ? 0u : 1u;
                const uint32_t v = 3u * t + (uint32_t)k;
                kmin[a] = min(kmin[a], min_key(p, v));
                kmax[a] = max(kmax[a], max_key(p, v));
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int a = 0; a < 3; ++a) {
            kmin[a] = min(kmin[a], (unsigned long long)__shfl_xor(kmin[a], off));
            kmax[a] = max(kmax[a], (unsigned long long)__shfl_xor(kmax[a], off));
        }
        bad |= (uint32_t)__shfl_xor((int)bad, off);
    }
    __shared__ unsigned long long s_key[4][6];
    __shared__ uint32_t s_bad[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int a = 0; a < 3; ++a) s_key[wave][a] = kmin[a], s_key[wave][3 + a] = kmax[a];
        s_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            for (int a = 0; a < 3; ++a) kmin[a] = min(kmin[a], s_key[w][a]), kmax[a] = max(kmax[a], s_key[w][3 + a]);
            bad |= s_bad[w];
        }
        for (int a = 0; a < 3; ++a) atomicMin(&red[a], kmin[a]), atomicMax(&red[3 + a], kmax[a]);
        if (bad) atomicOr(&red[6], 1ull);
    }
}

// Phase 2a: the leaf records' v0 / e1 / e2 (scene_rules.h: tri_record), in place in the packed array.
__global__ void __launch_bounds__(256) k_upd_records(uint32_t n_recs, uint8_t* __restrict__ tris, const float* __restrict__ wv) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_recs) return;
    const uint32_t g = packed_global_index(tris, r);
    if (g == kNoTri) return; // the empty scene's dummy record
    float* rec = packed_tri(tris, r);
    tri_record(wv + 9 * (size_t)g, rec, rec + 3, rec + 6);
}

// Phase 2b: one height level of the refit (scene_rules.h: refit_node). An inner child's exact box was stored one launch earlier.
__global__ void __launch_bounds__(128) k_upd_refit(uint32_t n, const uint32_t* __restrict__ level, BvhNode* __restrict__ nodes,
                                                    const uint8_t* __restrict__ tris, const float* __restrict__ wv, Box3* __restrict__ box,
                                                    float pad, unsigned long long* __restrict__ failed) {
    const uint32_t i = blockIdx.x * 128u + threadIdx.x;
    if (i >= n) return;
    const uint32_t ni = level[i];
    const BvhNode nd = nodes[ni];
    BvhNode q;
    const RefitResult res = refit_node(
        nd, [=](int32_t child) { return box[host_child_word((uint32_t)child)]; },
        [=](uint32_t r) { return wv + 9 * (size_t)packed_global_index(tris, r); }, pad, box[ni], q);
    if (res == kRefitEmpty) return;
    if (res == kRefitRefused) atomicOr(failed, 1ull);
    nodes[ni] = q;
}

// Phase 2c: the shading word of every triangle whose instance's table row moved (islot: the word of every instance).
__global__ void __launch_bounds__(256) k_upd_words(uint32_t n_tris, const uint32_t* __restrict__ tri_inst, const uint32_t* __restrict__ islot,
                                                    ShadeRec* __restrict__ shade) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tris) return;
    const uint32_t w = islot[tri_inst[t]];
    if (shade[t].instance != w) shade[t].instance = w;
}

// Phase 2d: the shading normals n0..n2, re-gathered through the kept indices.
__global__ void __launch_bounds__(256) k_upd_normals(uint32_t n_tris, const uint32_t* __restrict__ idx, const float* __restrict__ nrm,
                                                      ShadeRec* __restrict__ shade) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tris) return;
    shade_normals(shade[t], idx + 3 * (size_t)t, nrm);
}

// the 16 floats of every instance's transform, as k_upd_transform reads them
std::vector<float> transforms_of(const rt_instance* inst, size_t n) {
    std::vector<float> xf(16 * n);
    for (size_t i = 0; i < n; ++i) std::memcpy(&xf[16 * i], inst[i].transform, 64);
    return xf;
}

// The end of an accepted update, host or device: the instances and their rows as they are now, the statistics; a device scene's host copy lags.
void commit_update(rt_scene* s, const std::vector<rt_instance>& inst, const std::vector<uint32_t>& slot, const rt_update_stats& done, rt_update_stats* stats) {
    s->upd->inst_slot = slot, s->upd->instances = inst, s->upd->host_stale = s->device >= 0;
    if (stats) *stats = done;
}

// ---- host-only scenes: the same update in host arithmetic (the CPU reference of the device path) ---------------------------------------
int update_host(rt_scene* s, const std::vector<rt_instance>& inst, const rt_scene_update_desc* u, rt_update_stats* stats) {
    SceneUpdate& up = *s->upd;
    HostScene& hs = s->hs;
    const uint32_t T = (uint32_t)up.tri_instance.size();
    const bool new_pos = u->n_vertices && u->positions, new_nrm = u->n_vertices && u->normals;
    // phase 1: the world-space vertices, their bounds and the pad, or a refusal
    std::vector<float> wv;
    world_vertices(T, up.indices.data(), up.tri_instance.data(), inst.data(), new_pos ? u->positions : up.positions.data(), wv);
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, pad = hs.pad;
    std::string err;
    if (T && !world_bounds(wv, lo, hi, pad, err)) return fail(RT_ERR_INVALID, err);
    // phase 2: the update is accepted
    HostScene next = hs; // (a quantisation failure below leaves the scene as it was)
    if (T) {
        next.wverts.swap(wv);
        std::memcpy(next.bounds_lo, lo, 12), std::memcpy(next.bounds_hi, hi, 12);
        next.pad = pad;
        std::vector<float> box;
        if (!refit_host(next, up.level_nodes, box, err)) return fail(RT_ERR_INVALID, err);
    }
    std::vector<uint32_t> slot;
    shading_rows(inst.data(), (uint32_t)inst.size(), up.inst_use, hs.packed_mat, next.inst, slot);
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t i = up.tri_instance[t];
        next.shade[t].instance = shading_word(hs.packed_mat, slot[i], inst[i].material, i);
        if (new_nrm) shade_normals(next.shade[t], &up.indices[3 * (size_t)t], u->normals);
    }
    hs = std::move(next);
    if (new_pos) up.positions.assign(u->positions, u->positions + 3 * (size_t)up.n_vertices);
    if (new_nrm) up.normals.assign(u->normals, u->normals + 3 * (size_t)up.n_vertices);
    commit_update(s, inst, slot, rt_update_stats{0.0, 0u, T ? (uint32_t)up.level_nodes.size() : 0u}, stats);
    return RT_OK;
}

// ---- device scenes -----------------------------------------------------------------------------------------------------------------------
template <bool WRITE>
void launch_transform(const SceneUpdate& up, uint32_t T, const float* pos, const float* xf) {
    hipLaunchKernelGGL(k_upd_transform<WRITE>, dim3((T + 255u) / 256u), dim3(256), 0, up.stream, T, pos, (const uint32_t*)up.d_idx.get(),
                       (const uint32_t*)up.d_tri_inst.get(), xf, up.d_wv.get(), up.d_red.get());
}

int update_device(rt_scene* s, const std::vector<rt_instance>& inst, const rt_scene_update_desc* u, rt_update_stats* stats) {
    SceneUpdate& up = *s->upd;
    HostScene& hs = s->hs;
    HIPCHK(hipSetDevice(s->device));
    const uint32_t T = (uint32_t)(hs.wverts.size() / 9), I = (uint32_t)inst.size();
    const uint32_t n_recs = s->dev.n_tris ? (uint32_t)hs.tris.size() : 0u; // (hs.tris.size() never changes: the leaf records are kept)
    const uint32_t g256 = (T + 255u) / 256u;
    hipStream_t st = up.stream;
    unsigned long long* h_red = up.h_red.get();
    rt_update_stats done{};
    HIPCHK(hipEventRecord(up.ev0, st));
    // what the update brings goes into the staging buffers
    const bool new_xf = u->n_instances != 0, new_pos = u->n_vertices && u->positions, new_nrm = u->n_vertices && u->normals;
    const std::vector<float> xf = new_xf ? transforms_of(inst.data(), I) : std::vector<float>();
    if (new_xf) HIPCHK(hipMemcpyAsync(up.d_xf_stage.get(), xf.data(), xf.size() * 4, hipMemcpyHostToDevice, st));
    if (new_pos) HIPCHK(hipMemcpyAsync(up.d_pos_stage.get(), u->positions, 12 * (size_t)up.n_vertices, hipMemcpyHostToDevice, st));
    const float* xf_new = new_xf ? up.d_xf_stage.get() : up.d_xf.get();
    const float* pos_new = new_pos ? up.d_pos_stage.get() : up.d_pos.get();
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, pad = hs.pad;
    if (T) {
        // phase 1: the world-space vertices, their bounds and the pad, or a refusal
        for (int a = 0; a < 3; ++a) h_red[a] = ~0ull, h_red[3 + a] = 0ull;
        h_red[6] = h_red[7] = 0ull;
        HIPCHK(hipMemcpyAsync(up.d_red.get(), h_red, kRedWords * 8, hipMemcpyHostToDevice, st));
        if (up.keep_previous) launch_transform<false>(up, T, pos_new, xf_new); // test first, write after (below): the current vertices are still needed as the previous ones
        else launch_transform<true>(up, T, pos_new, xf_new);
        ++done.launches;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_red, up.d_red.get(), kRedWords * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int a = 0; a < 3; ++a) lo[a] = key_value(h_red[a]), hi[a] = key_value(h_red[3 + a]);
        std::string err;
        const bool ok = h_red[6] == 0 ? scene_padding(lo, hi, pad, err) : (err = "non-finite world-space vertex", false);
        if (!ok && up.keep_previous) return fail(RT_ERR_INVALID, err); // refused: nothing was written
        if (!ok) { // refused: the scratch vertices go back to the scene's own, nothing else was written
            launch_transform<true>(up, T, up.d_pos.get(), up.d_xf.get());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
            return fail(RT_ERR_INVALID, err);
        }
        if (up.keep_previous) { // accepted: the current vertices become the previous ones (a pointer swap), the new ones are written over the older copy
            std::swap(up.d_wv, up.d_wv_prev);
            launch_transform<true>(up, T, pos_new, xf_new); // (its reduction repeats the one read above: words 0 .. 6, nobody reads them again)
            ++done.launches;
            HIPCHK(hipGetLastError());
        }
    }
    // phase 2: the update is accepted
    if (new_xf) std::swap(up.d_xf, up.d_xf_stage);
    if (new_pos) std::swap(up.d_pos, up.d_pos_stage);
    if (T) { // the leaf records, then the nodes level by level
        hipLaunchKernelGGL(k_upd_records, dim3((n_recs + 255u) / 256u), dim3(256), 0, st, n_recs, s->d_tris.get(), (const float*)up.d_wv.get());
        ++done.launches;
        h_red[7] = 0ull;
        HIPCHK(hipMemcpyAsync(up.d_red.get() + 7, h_red + 7, 8, hipMemcpyHostToDevice, st));
        for (size_t h = 0; h + 1 < up.level_start.size(); ++h) {
            const uint32_t n = up.level_start[h + 1] - up.level_start[h];
            if (!n) continue;
            hipLaunchKernelGGL(k_upd_refit, dim3((n + 127u) / 128u), dim3(128), 0, st, n, (const uint32_t*)(up.d_levels.get() + up.level_start[h]),
                               s->d_nodes.get(), (const uint8_t*)s->d_tris.get(), (const float*)up.d_wv.get(), (Box3*)up.d_box.get(), pad, up.d_red.get() + 7);
            ++done.launches;
            done.refit_nodes += n;
        }
        HIPCHK(hipGetLastError());
    }
    // the instance table, and the shading records where its rows moved / where normals came
    std::vector<InstRec> rows;
    std::vector<uint32_t> slot, words;
    shading_rows(inst.data(), I, up.inst_use, hs.packed_mat, rows, slot);
    const bool moved = slot != up.inst_slot;
    if (new_xf) {
        if (rows.size() > scene_inst_capacity(s)) return fail(RT_ERR_INVALID, "internal: instance table capacity exceeded");
        HIPCHK(hipMemcpyAsync(s->d_inst.get(), rows.data(), rows.size() * sizeof(InstRec), hipMemcpyHostToDevice, st));
    }
    if (moved && T) {
        words.resize(I);
        for (uint32_t i = 0; i < I; ++i) words[i] = shading_word(hs.packed_mat, slot[i], inst[i].material, i);
        HIPCHK(hipMemcpyAsync(up.d_islot.get(), words.data(), (size_t)I * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_upd_words, dim3(g256), dim3(256), 0, st, T, (const uint32_t*)up.d_tri_inst.get(), (const uint32_t*)up.d_islot.get(), s->d_shade.get());
        ++done.launches;
    }
    if (new_nrm && T) {
        HIPCHK(hipMemcpyAsync(up.d_pos_stage.get(), u->normals, 12 * (size_t)up.n_vertices, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_upd_normals, dim3(g256), dim3(256), 0, st, T, (const uint32_t*)up.d_idx.get(), (const float*)up.d_pos_stage.get(), s->d_shade.get());
        ++done.launches;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(up.ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (T) HIPCHK(hipMemcpy(h_red + 7, up.d_red.get() + 7, 8, hipMemcpyDeviceToHost));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, up.ev0, up.ev1));
    done.device_ms = (double)ms;
    commit_update(s, inst, slot, done, stats);
    if (T && h_red[7]) { // cannot happen within the padded bounds rt_scene_create accepts; reported all the same
        ++s->generation;
        return fail(RT_ERR_INVALID, "internal: a refit node's child boxes could not be quantised");
    }
    hs.inst = rows;
    if (T) std::memcpy(hs.bounds_lo, lo, 12), std::memcpy(hs.bounds_hi, hi, 12), hs.pad = pad;
    scene_scalars(hs, s->dev);
    return RT_OK;
}

} // namespace

uint32_t scene_inst_capacity(const rt_scene* s) {
    return (uint32_t)std::max<size_t>(std::max<size_t>(s->hs.inst.size(), s->upd ? s->upd->instances.size() : 0), 1);
}

int init_scene_update(rt_scene* s, const rt_scene_desc* d, bool keep_previous) {
    s->upd.reset(new SceneUpdate());
    SceneUpdate& u = *s->upd;
    u.keep_previous = keep_previous;
    const uint32_t T = d->n_triangles, I = d->n_instances, V = d->n_vertices;
    u.n_vertices = V;
    u.instances.assign(d->instances, d->instances + I);
    u.inst_use.assign(I, 0);
    for (uint32_t t = 0; t < T; ++t) u.inst_use[d->tri_instance[t]]++;
    {
        std::vector<InstRec> rows;
        shading_rows(d->instances, I, u.inst_use, s->hs.packed_mat, rows, u.inst_slot);
    }
    node_levels(s->hs.nodes, u.level_nodes, u.level_start);
    if (s->device < 0) {
        if (T) {
            u.positions.assign(d->positions, d->positions + 3 * (size_t)V);
            u.normals.assign(d->normals, d->normals + 3 * (size_t)V);
        }
        u.indices.assign(d->indices, d->indices + 3 * (size_t)T);
        u.tri_instance.assign(d->tri_instance, d->tri_instance + T);
        return RT_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    SceneAlloc& al = s->alloc;
    uint64_t& b = s->device_bytes;
    const size_t n_nodes = s->hs.nodes.size();
    const float* wv = T ? s->hs.wverts.data() : nullptr; // (before the first update previous == current)
    const std::vector<float> xf = transforms_of(d->instances, I);
    int rc = u.d_pos.upload(al, T ? d->positions : nullptr, 3 * (size_t)V, b);
    if (!rc) rc = u.d_pos_stage.upload(al, nullptr, 3 * (size_t)V, b);
    if (!rc) rc = u.d_idx.upload(al, d->indices, 3 * (size_t)T, b);
    if (!rc) rc = u.d_tri_inst.upload(al, d->tri_instance, T, b);
    if (!rc) rc = u.d_xf.upload(al, xf, b);
    if (!rc) rc = u.d_xf_stage.upload(al, nullptr, xf.size(), b);
    if (!rc) rc = u.d_islot.upload(al, nullptr, I, b);
    if (!rc) rc = u.d_wv.upload(al, wv, 9 * (size_t)T, b);
    if (!rc && keep_previous && T) rc = u.d_wv_prev.upload(al, wv, 9 * (size_t)T, b); // + 36 bytes per triangle
    if (!rc) rc = u.d_box.upload(al, nullptr, 6 * n_nodes, b);
    if (!rc) rc = u.d_levels.upload(al, u.level_nodes, b);
    if (!rc) rc = u.d_red.upload(al, nullptr, kRedWords, b);
    if (rc) return rc;
    HIPCHK(al.pinned((void**)&u.h_red.p, kRedWords * 8));
    HIPCHK(hipStreamCreateWithFlags(&u.stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&u.ev0));
    HIPCHK(hipEventCreate(&u.ev1));
    HIPCHK(hipMemset(u.d_box.get(), 0, 24 * std::max<size_t>(n_nodes, 1)));
    return RT_OK;
}

int sync_host_copy(const rt_scene* cs) {
    rt_scene* s = const_cast<rt_scene*>(cs); // the host copy is a cache of the device's scene
    if (!s->upd || !s->upd->host_stale) return RT_OK;
    return no_throw([&]() -> int {
        SceneUpdate& up = *s->upd;
        HostScene& hs = s->hs;
        HIPCHK(hipSetDevice(s->device));
        std::vector<BvhNode> nodes(hs.nodes.size());
        std::vector<uint8_t> packed(packed_tri_bytes(hs.tris.size()));
        std::vector<float> wv(hs.wverts.size()), box(6 * hs.nodes.size());
        std::vector<ShadeRec> shade(hs.shade.size());
        HIPCHK(hipMemcpy(nodes.data(), s->d_nodes.get(), nodes.size() * sizeof(BvhNode), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(packed.data(), s->d_tris.get(), packed.size(), hipMemcpyDeviceToHost));
        if (!wv.empty()) HIPCHK(hipMemcpy(wv.data(), up.d_wv.get(), wv.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(box.data(), up.d_box.get(), box.size() * 4, hipMemcpyDeviceToHost));
        if (!shade.empty()) HIPCHK(hipMemcpy(shade.data(), s->d_shade.get(), shade.size() * sizeof(ShadeRec), hipMemcpyDeviceToHost));
        host_nodes(nodes);
        unpack_tris(packed, hs.tris);
        hs.nodes.swap(nodes);
        hs.wverts.swap(wv);
        hs.shade.swap(shade);
        record_boxes(hs);
        if (!hs.wverts.empty()) hs.sah_cost = refit_sah_cost(hs, box);
        up.host_stale = false;
        return (int)RT_OK;
    });
}

} // namespace rtlib

extern "C" int rt_scene_update(rt_scene* s, const rt_scene_update_desc* u, rt_update_stats* stats) {
    if (!s || !u) return fail(RT_ERR_INVALID, "null argument");
    if (!s->upd) return fail(RT_ERR_INVALID, "the scene was not created updatable (rt_scene_create_ex with RT_SCENE_UPDATABLE)");
    if (s->frames_pending) return fail(RT_ERR_INVALID, "a renderer of the scene has a frame in flight (rt_render_frame_end first)");
    const SceneUpdate& up = *s->upd;
    if (u->n_instances && u->n_instances != up.instances.size()) return fail(RT_ERR_INVALID, "n_instances must be 0 or the scene's");
    if (u->n_instances && !u->instances) return fail(RT_ERR_INVALID, "null instance array");
    if (u->n_vertices && u->n_vertices != up.n_vertices) return fail(RT_ERR_INVALID, "n_vertices must be 0 or the scene's");
    if (u->n_vertices && !u->positions && !u->normals) return fail(RT_ERR_INVALID, "n_vertices given with neither positions nor normals");
    for (uint32_t i = 0; i < u->n_instances; ++i)
        if (u->instances[i].material != up.instances[i].material) return fail(RT_ERR_INVALID, "an update cannot change an instance's material");
    if (!s->readers.empty()) { // the G-buffer, query and lightmap launches still reading the scene, on any stream (rt_scene::readers), finish before anything is rewritten
        HIPCHK(hipSetDevice(s->device));
        for (const auto& se : s->readers) HIPCHK(hipEventSynchronize(se.second));
    }
    return no_throw([&]() -> int {
        std::vector<rt_instance> inst = up.instances;
        for (uint32_t i = 0; i < u->n_instances; ++i) inst[i] = u->instances[i];
        rt_update_stats local{};
        const int rc = s->device < 0 ? update_host(s, inst, u, &local) : update_device(s, inst, u, &local);
        if (rc != RT_OK) return rc;
        ++s->generation;
        if (stats) *stats = local;
        return (int)RT_OK;
    });
}
