// rt_update.hip — dynamic scenes: what rt_scene_create_ex keeps for RT_SCENE_UPDATABLE, rt_scene_update and its kernels, and the lazy
// refresh of the host copy. A unit of its own, so that the render kernels (rt_frame.hip) compile to the same code as without it.
//
// An update keeps the BVH's topology (child words, leaf codes, node order) and recomputes everything geometric in place, in two phases:
//   1. k_upd_transform: every triangle's world-space vertices, with the host builder's expression ((m0*x + m4*y) + m8*z) + m12
//      (scene_build.cpp: world_vertices, -ffp-contract=off), into the scratch array `wv`; in the same pass the scene's bounds as ordered keys that also
//      carry the first occurrence (the host's std::min / std::max keep the first of equal values: the sign of a zero bound depends on it)
//      and a non-finite flag. The host reads back 7 words and applies rt_scene_create's test. A refusal restores `wv` and stops here:
//      nothing else of the scene has been written.
//   2. k_upd_records rewrites v0 / e1 / e2 of every leaf record, k_upd_refit the nodes, one launch per height level (a node's children lie in
//      lower levels, so the kernel boundary is the only hand-off between workgroups: no atomics, no fences), k_upd_words / k_upd_normals the
//      shading records where the instance table's rows moved / where normals were given.
// Every write lands in a buffer that exists since rt_scene_create: no device pointer of SceneDev changes.
#include "bvh_quantise.h"
#include "rt_internal.h"

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
                const float p = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[a], x), __fmul_rn(m[4 + a], y)), __fmul_rn(m[8 + a], z)), m[12 + a]);
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

// Phase 2a: the leaf records' v0, e1 = v1 - v0, e2 = v2 - v0 (kTriBytes layout: v0.xyz e1.xyz e2.xyz global_index), in place.
__global__ void __launch_bounds__(256) k_upd_records(uint32_t n_recs, uint8_t* __restrict__ tris, const float* __restrict__ wv) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_recs) return;
    float* rec = reinterpret_cast<float*>(tris + (size_t)r * kTriBytes);
    const uint32_t g = reinterpret_cast<const uint32_t*>(rec)[9];
    if (g == kNoTri) return; // the empty scene's dummy record
    const float* w = wv + 9 * (size_t)g;
    for (int a = 0; a < 3; ++a) {
        rec[a] = w[a];
        rec[3 + a] = __fsub_rn(w[3 + a], w[a]);
        rec[6 + a] = __fsub_rn(w[6 + a], w[a]);
    }
}

// Phase 2b: one height level of the refit. A node's exact child boxes: the union of a leaf's triangles' boxes (every record bounds its
// whole triangle), or the exact box an inner child stored one launch earlier. Words 0..11 are re-quantised with the new pad; the child
// words stay.
__global__ void __launch_bounds__(128) k_upd_refit(uint32_t n, const uint32_t* __restrict__ level, BvhNode* __restrict__ nodes,
                                                    const uint8_t* __restrict__ tris, const float* __restrict__ wv, Box3* __restrict__ box,
                                                    float pad, unsigned long long* __restrict__ failed) {
    const uint32_t i = blockIdx.x * 128u + threadIdx.x;
    if (i >= n) return;
    const uint32_t ni = level[i];
    BvhNode nd = nodes[ni];
    Box3 kb[4];
    int nk = 0;
    for (int k = 0; k < 4 && nd.child[k] != kChildEmpty; ++k, ++nk) {
        const int32_t c = nd.child[k];
        if (c >= 0) {
            kb[k] = box[(uint32_t)c / 64u]; // (the device's child words are byte offsets)
        } else {
            const LeafRange leaf = leaf_range(c);
            for (int a = 0; a < 3; ++a) kb[k].lo[a] = INFINITY, kb[k].hi[a] = -INFINITY;
            for (uint32_t r = leaf.first; r < leaf.first + leaf.count; ++r) {
                const uint32_t g = *reinterpret_cast<const uint32_t*>(tris + (size_t)r * kTriBytes + 36);
                const float* w = wv + 9 * (size_t)g;
                for (int a = 0; a < 3; ++a) {
                    kb[k].lo[a] = fminf(kb[k].lo[a], fminf(w[a], fminf(w[3 + a], w[6 + a])));
                    kb[k].hi[a] = fmaxf(kb[k].hi[a], fmaxf(w[a], fmaxf(w[3 + a], w[6 + a])));
                }
            }
        }
    }
    if (nk == 0) return;
    Box3 u = kb[0];
    for (int k = 1; k < nk; ++k)
        for (int a = 0; a < 3; ++a) u.lo[a] = fminf(u.lo[a], kb[k].lo[a]), u.hi[a] = fmaxf(u.hi[a], kb[k].hi[a]);
    box[ni] = u;
    BvhNode q;
    if (!quantise_node(q, nk, kb, pad)) atomicOr(failed, 1ull);
    for (int k = 0; k < 4; ++k) q.child[k] = nd.child[k];
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
    ShadeRec& s = shade[t];
    float* dst[3] = {s.n0, s.n1, s.n2};
    for (int k = 0; k < 3; ++k) {
        const uint32_t vi = idx[3 * (size_t)t + k];
        for (int a = 0; a < 3; ++a) dst[k][a] = nrm[3 * (size_t)vi + a];
    }
}

template <typename T>
hipError_t dev_alloc(T** p, size_t count, uint64_t& bytes) {
    const size_t b = std::max<size_t>(count, 1) * sizeof(T);
    const hipError_t e = hipMalloc((void**)p, b);
    if (e == hipSuccess) bytes += b;
    return e;
}

uint32_t shading_word(const rt_scene* s, uint32_t inst) {
    const SceneUpdate& u = *s->upd;
    return s->hs.packed_mat ? (u.inst_slot[inst] | (u.instances[inst].material << kPackedInstBits)) : inst;
}

// the new instance table; returns whether any instance's row moved
bool regroup(rt_scene* s, const std::vector<rt_instance>& inst, std::vector<InstRec>& rows, std::vector<uint32_t>& slot) {
    shading_rows(inst.data(), (uint32_t)inst.size(), s->upd->inst_use, s->hs.packed_mat, rows, slot);
    return slot != s->upd->inst_slot;
}

// ---- host-only scenes: the same update in host arithmetic (the CPU reference of the device path) ---------------------------------------
int update_host(rt_scene* s, const std::vector<rt_instance>& inst, const rt_scene_update_desc* u, rt_update_stats* stats) {
    SceneUpdate& up = *s->upd;
    HostScene& hs = s->hs;
    const uint32_t T = (uint32_t)up.tri_instance.size();
    const float* pos = (u->n_vertices && u->positions) ? u->positions : up.positions.data();
    std::vector<float> wv;
    world_vertices(T, up.indices.data(), up.tri_instance.data(), inst.data(), pos, wv);
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, pad = hs.pad;
    std::string err;
    if (T && !world_bounds(wv, lo, hi, pad, err)) return fail(RT_ERR_INVALID, err);
    // accepted: from here on the scene changes
    HostScene next = hs; // (a quantisation failure below leaves the scene as it was)
    if (T) {
        next.wverts.swap(wv);
        std::memcpy(next.bounds_lo, lo, 12), std::memcpy(next.bounds_hi, hi, 12);
        next.pad = pad;
        std::vector<float> box;
        if (!refit_host(next, up.level_nodes, box, err)) return fail(RT_ERR_INVALID, err);
    }
    std::vector<InstRec> rows;
    std::vector<uint32_t> slot;
    regroup(s, inst, rows, slot);
    next.inst = rows;
    if (u->n_vertices && u->normals)
        for (uint32_t t = 0; t < T; ++t) {
            ShadeRec& sr = next.shade[t];
            float* dst[3] = {sr.n0, sr.n1, sr.n2};
            for (int k = 0; k < 3; ++k) std::memcpy(dst[k], u->normals + 3 * (size_t)up.indices[3 * (size_t)t + k], 12);
        }
    hs = std::move(next);
    up.inst_slot = slot;
    up.instances = inst;
    for (uint32_t t = 0; t < T; ++t) hs.shade[t].instance = shading_word(s, up.tri_instance[t]);
    if (u->n_vertices && u->positions) up.positions.assign(u->positions, u->positions + 3 * (size_t)up.n_vertices);
    if (u->n_vertices && u->normals) up.normals.assign(u->normals, u->normals + 3 * (size_t)up.n_vertices);
    if (stats) stats->device_ms = 0.0, stats->launches = 0, stats->refit_nodes = T ? (uint32_t)up.level_nodes.size() : 0u;
    return RT_OK;
}

// ---- device scenes -----------------------------------------------------------------------------------------------------------------------
int update_device(rt_scene* s, const std::vector<rt_instance>& inst, const rt_scene_update_desc* u, rt_update_stats* stats) {
    SceneUpdate& up = *s->upd;
    HostScene& hs = s->hs;
    HIPCHK(hipSetDevice(s->device));
    const uint32_t T = (uint32_t)(hs.wverts.size() / 9), I = (uint32_t)inst.size();
    const uint32_t n_recs = s->dev.n_tris ? (uint32_t)hs.tris.size() : 0u; // (hs.tris.size() never changes: the leaf records are kept)
    hipStream_t st = up.stream;
    uint32_t launches = 0;
    HIPCHK(hipEventRecord(up.ev0, st));
    const bool new_xf = u->n_instances != 0, new_pos = u->n_vertices && u->positions;
    std::vector<float> xf;
    if (new_xf) {
        xf.resize(16 * (size_t)I);
        for (uint32_t i = 0; i < I; ++i) std::memcpy(&xf[16 * (size_t)i], inst[i].transform, 64);
        HIPCHK(hipMemcpyAsync(up.d_xf_stage, xf.data(), xf.size() * 4, hipMemcpyHostToDevice, st));
    }
    if (new_pos) HIPCHK(hipMemcpyAsync(up.d_pos_stage, u->positions, 12 * (size_t)up.n_vertices, hipMemcpyHostToDevice, st));
    const float* xf_new = new_xf ? up.d_xf_stage : up.d_xf;
    const float* pos_new = new_pos ? up.d_pos_stage : up.d_pos;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, pad = hs.pad;
    const uint32_t g256 = (T + 255u) / 256u;
    if (T) {
        // phase 1
        for (int a = 0; a < 3; ++a) up.h_red[a] = ~0ull, up.h_red[3 + a] = 0ull;
        up.h_red[6] = up.h_red[7] = 0ull;
        HIPCHK(hipMemcpyAsync(up.d_red, up.h_red, kRedWords * 8, hipMemcpyHostToDevice, st));
        if (up.keep_previous) // test first, write after (below): the current vertices are still needed as the previous ones
            hipLaunchKernelGGL(k_upd_transform<false>, dim3(g256), dim3(256), 0, st, T, pos_new, (const uint32_t*)up.d_idx, (const uint32_t*)up.d_tri_inst, xf_new, up.d_wv, up.d_red);
        else
            hipLaunchKernelGGL(k_upd_transform<true>, dim3(g256), dim3(256), 0, st, T, pos_new, (const uint32_t*)up.d_idx, (const uint32_t*)up.d_tri_inst, xf_new, up.d_wv, up.d_red);
        ++launches;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(up.h_red, up.d_red, kRedWords * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int a = 0; a < 3; ++a) lo[a] = key_value(up.h_red[a]), hi[a] = key_value(up.h_red[3 + a]);
        std::string err;
        const bool ok = up.h_red[6] == 0 ? scene_padding(lo, hi, pad, err) : (err = "non-finite world-space vertex", false);
        if (!ok && up.keep_previous) return fail(RT_ERR_INVALID, err); // refused: nothing was written
        if (!ok) { // refused: the scratch vertices go back to the scene's own, nothing else was written
            hipLaunchKernelGGL(k_upd_transform<true>, dim3(g256), dim3(256), 0, st, T, (const float*)up.d_pos, (const uint32_t*)up.d_idx,
                               (const uint32_t*)up.d_tri_inst, (const float*)up.d_xf, up.d_wv, up.d_red);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
            return fail(RT_ERR_INVALID, err);
        }
        if (up.keep_previous) { // accepted: the current vertices become the previous ones (a pointer swap), the new ones are written over the older copy
            std::swap(up.d_wv, up.d_wv_prev);
            hipLaunchKernelGGL(k_upd_transform<true>, dim3(g256), dim3(256), 0, st, T, pos_new, (const uint32_t*)up.d_idx, (const uint32_t*)up.d_tri_inst, xf_new, up.d_wv,
                               up.d_red); // (its reduction repeats the one read above: words 0 .. 6, nobody reads them again)
            ++launches;
            HIPCHK(hipGetLastError());
        }
    }
    // phase 2: the update is accepted
    if (new_xf) std::swap(up.d_xf, up.d_xf_stage);
    if (new_pos) std::swap(up.d_pos, up.d_pos_stage);
    uint32_t refit_nodes = 0;
    if (T) {
        hipLaunchKernelGGL(k_upd_records, dim3((n_recs + 255u) / 256u), dim3(256), 0, st, n_recs, (uint8_t*)s->dev.tris, (const float*)up.d_wv);
        ++launches;
        up.h_red[7] = 0ull;
        HIPCHK(hipMemcpyAsync(up.d_red + 7, up.h_red + 7, 8, hipMemcpyHostToDevice, st));
        for (size_t h = 0; h + 1 < up.level_start.size(); ++h) {
            const uint32_t n = up.level_start[h + 1] - up.level_start[h];
            if (!n) continue;
            hipLaunchKernelGGL(k_upd_refit, dim3((n + 127u) / 128u), dim3(128), 0, st, n, (const uint32_t*)(up.d_levels + up.level_start[h]),
                               (BvhNode*)s->dev.nodes, (const uint8_t*)s->dev.tris, (const float*)up.d_wv, (Box3*)up.d_box, pad, up.d_red + 7);
            ++launches;
            refit_nodes += n;
        }
        HIPCHK(hipGetLastError());
    }
    std::vector<InstRec> rows;
    std::vector<uint32_t> slot;
    const bool moved = regroup(s, inst, rows, slot);
    if (new_xf) {
        if (rows.size() > scene_inst_capacity(s)) return fail(RT_ERR_INVALID, "internal: instance table capacity exceeded");
        HIPCHK(hipMemcpyAsync((void*)s->dev.inst, rows.data(), rows.size() * sizeof(InstRec), hipMemcpyHostToDevice, st));
    }
    up.inst_slot = slot;
    up.instances = inst;
    if (moved && T) {
        std::vector<uint32_t> words(I);
        for (uint32_t i = 0; i < I; ++i) words[i] = shading_word(s, i);
        HIPCHK(hipMemcpyAsync(up.d_islot, words.data(), (size_t)I * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_upd_words, dim3(g256), dim3(256), 0, st, T, (const uint32_t*)up.d_tri_inst, (const uint32_t*)up.d_islot,
                           (ShadeRec*)s->dev.shade);
        ++launches;
    }
    if (u->n_vertices && u->normals && T) {
        HIPCHK(hipMemcpyAsync(up.d_pos_stage, u->normals, 12 * (size_t)up.n_vertices, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_upd_normals, dim3(g256), dim3(256), 0, st, T, (const uint32_t*)up.d_idx, (const float*)up.d_pos_stage,
                           (ShadeRec*)s->dev.shade);
        ++launches;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(up.ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (T) {
        HIPCHK(hipMemcpy(up.h_red + 7, up.d_red + 7, 8, hipMemcpyDeviceToHost));
        if (up.h_red[7]) { // cannot happen within the padded bounds rt_scene_create accepts; reported all the same
            up.host_stale = true;
            ++s->generation;
            return fail(RT_ERR_INVALID, "internal: a refit node's child boxes could not be quantised");
        }
    }
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, up.ev0, up.ev1));
    hs.inst = rows;
    const bool stage = hs.packed_mat && hs.n_layers <= 65536u; // as rt_scene_create decides it
    s->dev.lds_nm = stage ? (uint32_t)std::min<size_t>(hs.inst.size(), kLdsNm) : 0u;
    if (T) {
        std::memcpy(hs.bounds_lo, lo, 12), std::memcpy(hs.bounds_hi, hi, 12);
        hs.pad = pad;
        scene_cells(hs, s->dev);
    }
    up.host_stale = true;
    if (stats) stats->device_ms = (double)ms, stats->launches = launches, stats->refit_nodes = refit_nodes;
    return RT_OK;
}

} // namespace

uint32_t scene_inst_capacity(const rt_scene* s) {
    return (uint32_t)std::max<size_t>(std::max<size_t>(s->hs.inst.size(), s->upd ? s->upd->instances.size() : 0), 1);
}

void free_scene_update(rt_scene* s) {
    SceneUpdate* u = s->upd;
    if (!u) return;
    if (s->device >= 0 && hipSetDevice(s->device) == hipSuccess) {
        for (void* p : {(void*)u->d_pos, (void*)u->d_pos_stage, (void*)u->d_idx, (void*)u->d_tri_inst, (void*)u->d_xf, (void*)u->d_xf_stage,
                        (void*)u->d_islot, (void*)u->d_wv, (void*)u->d_wv_prev, (void*)u->d_box, (void*)u->d_levels, (void*)u->d_red})
            if (p) (void)hipFree(p);
        if (u->h_red) (void)hipHostFree(u->h_red);
        if (u->ev0) (void)hipEventDestroy(u->ev0);
        if (u->ev1) (void)hipEventDestroy(u->ev1);
        if (u->stream) (void)hipStreamDestroy(u->stream);
    }
    delete u;
    s->upd = nullptr;
}

int init_scene_update(rt_scene* s, const rt_scene_desc* d, bool keep_previous) {
    s->upd = new SceneUpdate();
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
    uint64_t& b = s->device_bytes;
    const size_t n_nodes = s->hs.nodes.size();
    HIPCHK(dev_alloc(&u.d_pos, 3 * (size_t)V, b));
    HIPCHK(dev_alloc(&u.d_pos_stage, 3 * (size_t)V, b));
    HIPCHK(dev_alloc(&u.d_idx, 3 * (size_t)T, b));
    HIPCHK(dev_alloc(&u.d_tri_inst, T, b));
    HIPCHK(dev_alloc(&u.d_xf, 16 * (size_t)I, b));
    HIPCHK(dev_alloc(&u.d_xf_stage, 16 * (size_t)I, b));
    HIPCHK(dev_alloc(&u.d_islot, I, b));
    HIPCHK(dev_alloc(&u.d_wv, 9 * (size_t)T, b));
    if (keep_previous && T) HIPCHK(dev_alloc(&u.d_wv_prev, 9 * (size_t)T, b)); // + 36 bytes per triangle
    HIPCHK(dev_alloc(&u.d_box, 6 * n_nodes, b));
    HIPCHK(dev_alloc(&u.d_levels, u.level_nodes.size(), b));
    HIPCHK(dev_alloc(&u.d_red, kRedWords, b));
    HIPCHK(hipHostMalloc((void**)&u.h_red, kRedWords * 8));
    HIPCHK(hipStreamCreateWithFlags(&u.stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&u.ev0));
    HIPCHK(hipEventCreate(&u.ev1));
    if (T) {
        HIPCHK(hipMemcpy(u.d_pos, d->positions, 12 * (size_t)V, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(u.d_idx, d->indices, 12 * (size_t)T, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(u.d_tri_inst, d->tri_instance, 4 * (size_t)T, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(u.d_wv, s->hs.wverts.data(), 4 * s->hs.wverts.size(), hipMemcpyHostToDevice));
        if (keep_previous) HIPCHK(hipMemcpy(u.d_wv_prev, s->hs.wverts.data(), 4 * s->hs.wverts.size(), hipMemcpyHostToDevice)); // before the first update previous == current
    }
    if (I) {
        std::vector<float> xf(16 * (size_t)I);
        for (uint32_t i = 0; i < I; ++i) std::memcpy(&xf[16 * (size_t)i], d->instances[i].transform, 64);
        HIPCHK(hipMemcpy(u.d_xf, xf.data(), xf.size() * 4, hipMemcpyHostToDevice));
    }
    if (!u.level_nodes.empty())
        HIPCHK(hipMemcpy(u.d_levels, u.level_nodes.data(), 4 * u.level_nodes.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(u.d_box, 0, 24 * std::max<size_t>(n_nodes, 1)));
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
        std::vector<uint8_t> packed(hs.tris.size() * (size_t)kTriBytes);
        std::vector<float> wv(hs.wverts.size()), box(6 * hs.nodes.size());
        std::vector<ShadeRec> shade(hs.shade.size());
        HIPCHK(hipMemcpy(nodes.data(), s->dev.nodes, nodes.size() * sizeof(BvhNode), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(packed.data(), s->dev.tris, packed.size(), hipMemcpyDeviceToHost));
        if (!wv.empty()) HIPCHK(hipMemcpy(wv.data(), up.d_wv, wv.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(box.data(), up.d_box, box.size() * 4, hipMemcpyDeviceToHost));
        if (!shade.empty()) HIPCHK(hipMemcpy(shade.data(), s->dev.shade, shade.size() * sizeof(ShadeRec), hipMemcpyDeviceToHost));
        for (BvhNode& n : nodes)
            for (int k = 0; k < 4; ++k)
                if (n.child[k] >= 0) n.child[k] /= 64;
        for (size_t r = 0; r < hs.tris.size(); ++r) std::memcpy(&hs.tris[r], packed.data() + r * kTriBytes, kTriBytes);
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
    if (!s->ev_gbuffer.empty()) { // G-buffer and ray-query launches still reading the scene (rt_scene_gbuffer_device, rt_trace_rays_device, any stream) finish before anything is rewritten
        HIPCHK(hipSetDevice(s->device));
        for (const auto& se : s->ev_gbuffer) HIPCHK(hipEventSynchronize(se.second));
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
