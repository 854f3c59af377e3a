// rt_lightmap.hip — lightmap baking: rt_lightmap_create / _destroy, rt_lightmap_texels[_device], rt_lightmap_bake[_device] and their kernels.
// The atlas-side half of a lightmap bake around one gather query (rt_path_gather.hip, called through its public entry point): which triangle
// owns a texel (k_lm_owner), where the texel lies on it and with which shading normal, and the states of its entries (k_lm_texels), the mean
// of the entries' radiances (k_lm_resolve) and the filling of the gutters (k_lm_dilate). The arithmetic is the contract stated at
// rt_lightmap_bake in include/rt_mi355x.h; the numpy model that pins it bit for bit is tests/test_lightmap.py. No traversal, no LDS, no
// float atomics in this unit: the owner plane is an integer minimum, the statistics are ballots and integer sums.
#include "rt_internal.h"
#include "rt_device.h"

struct rt_lightmap {
    rt_scene* scene = nullptr;
    int device = -1;
    int32_t width = 0, height = 0;
    uint32_t max_repeats = 0;
    uint32_t n_tris = 0;
    uint32_t bands = 1;              // waves per triangle in k_lm_owner: the largest clamped box cut into row bands (lm_bands)
    float* d_uv = nullptr;           // 6 floats per triangle
    float* d_wv = nullptr;           // a scene without RT_SCENE_UPDATABLE: its world-space vertices, 9 floats per triangle
    uint32_t* d_owner = nullptr;     // per texel
    float* d_pos = nullptr;          // 3 floats per entry (max_repeats entries per texel)
    float* d_nrm = nullptr;
    uint32_t* d_state = nullptr;     // per entry
    float* d_rad = nullptr;          // 3 floats per entry
    uint32_t* d_rays = nullptr;      // per entry
    float4* d_plane[2] = {nullptr, nullptr};
    rt_lightmap_stats* d_stats = nullptr;
    hipStream_t stream = nullptr;    // the host forms run here
    hipEvent_t ev_last = nullptr;    // recorded behind every call: the next call's stream waits for it
    bool recorded = false;
};

namespace rt {

constexpr uint32_t kLmBlock = 256;     // k_lm_owner (four triangle bands), k_lm_texels
constexpr uint32_t kLmStatBlock = 64;  // k_lm_resolve, k_lm_dilate: one wave per workgroup, so a wave's ballot is the workgroup's count
constexpr uint32_t kLmLaneTexels = 16, kLmWaveTexels = kLmLaneTexels * kLmStatBlock; // ... and 1,024 texels per wave: one atomic per counter for them
constexpr uint32_t kLmBandTexels = 4096; // box texels one wave of k_lm_owner strides at most where bands can still be added: 64 per lane
constexpr uint32_t kLmMaxWaves = 1u << 30;

// ---- coverage: the one copy of the edge rule, used by k_lm_owner and k_lm_texels alike ---------------------------------------------------
struct P2 {
    float x, y;
};
// E(A, B, q) = (B.x - A.x) * (q.y - A.y) - (B.y - A.y) * (q.x - A.x), five R1 operations, never contracted
RT_DEV float lm_E(P2 a, P2 b, P2 q) {
    return __fsub_rn(__fmul_rn(__fsub_rn(b.x, a.x), __fsub_rn(q.y, a.y)), __fmul_rn(__fsub_rn(b.y, a.y), __fsub_rn(q.x, a.x)));
}
// the order of two corners: x, then y
RT_DEV bool lm_first(P2 a, P2 b) { return a.x < b.x || (a.x == b.x && a.y <= b.y); }
// the value of the directed edge i -> j at q, evaluated from the corner that comes first: the two triangles sharing an edge see exact negatives
RT_DEV float lm_edge(P2 i, P2 j, P2 q) { return lm_first(i, j) ? lm_E(i, j, q) : -lm_E(j, i, q); }

struct LmTri {
    P2 p[3];
    float area;
    bool ok; // six finite coordinates and an area that is not zero (a NaN area passes here and covers nothing below)
};
RT_DEV LmTri lm_tri(const float* __restrict__ uv, uint32_t t, float wf, float hf) {
    const float* c = uv + 6 * (size_t)t;
    LmTri r;
    bool fin = true;
    for (int k = 0; k < 3; ++k) {
        r.p[k].x = __fmul_rn(c[2 * k], wf), r.p[k].y = __fmul_rn(c[2 * k + 1], hf);
        fin = fin && __builtin_isfinite(r.p[k].x) && __builtin_isfinite(r.p[k].y);
    }
    r.area = lm_edge(r.p[0], r.p[1], r.p[2]);
    r.ok = fin && r.area != 0.0f;
    return r;
}
// PRE: t.ok. e1, e2: the edge values the barycentrics are made of
RT_DEV bool lm_covers(const LmTri& t, int32_t x, int32_t y, float& e1, float& e2) {
    const P2 c = {(float)x + 0.5f, (float)y + 0.5f};
    const float e0 = lm_edge(t.p[1], t.p[2], c);
    e1 = lm_edge(t.p[2], t.p[0], c);
    e2 = lm_edge(t.p[0], t.p[1], c);
    if (t.area > 0.0f) return e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f;
    if (t.area < 0.0f) return e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f;
    return false;
}

// The texels whose centres lie inside [lo, hi] on one axis of n texels, clamped in floating point before the conversion: [first, last], empty
// when last < first. A centre k + 0.5 lies inside iff lo - 0.5 <= k <= hi - 0.5; the roundings of the two subtractions only widen the range
// (every integer up to 8192 is an fp32 value and rounding is monotone). PRE: lo, hi finite.
struct LmSpan {
    int32_t first, last;
};
__host__ __device__ inline LmSpan lm_span(float lo, float hi, int32_t n) {
    const float a = fminf(fmaxf(lo - 0.5f, 0.0f), (float)n);
    const float b = fminf(fmaxf(hi - 0.5f, -1.0f), (float)(n - 1));
    return {(int32_t)a, (int32_t)floorf(b)};
}

// One wave per (triangle, row band): the triangle's clamped box is cut into `bands` bands of whole rows, and the lanes stride a band's texels
// row-major, 64 at a time. A covering lane takes the texel for its triangle unless a lower index has it (the plane starts as all ones).
__global__ void __launch_bounds__(kLmBlock) k_lm_owner(const float* __restrict__ uv, uint32_t n_tris, int32_t W, int32_t H, uint32_t bands,
                                                        uint32_t* __restrict__ owner) {
    const uint32_t wave = blockIdx.x * (kLmBlock / 64u) + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    const uint32_t tri = wave / bands, band = wave % bands;
    if (tri >= n_tris) return;
    const LmTri t = lm_tri(uv, tri, (float)W, (float)H);
    if (!t.ok) return;
    const LmSpan sx = lm_span(fminf(fminf(t.p[0].x, t.p[1].x), t.p[2].x), fmaxf(fmaxf(t.p[0].x, t.p[1].x), t.p[2].x), W);
    const LmSpan sy = lm_span(fminf(fminf(t.p[0].y, t.p[1].y), t.p[2].y), fmaxf(fmaxf(t.p[0].y, t.p[1].y), t.p[2].y), H);
    if (sx.last < sx.first || sy.last < sy.first) return;
    const uint32_t bw = (uint32_t)(sx.last - sx.first + 1), bh = (uint32_t)(sy.last - sy.first + 1); // at most W, H: 8192 each
    const uint32_t rows = (bh + bands - 1u) / bands, r0 = band * rows;
    if (r0 >= bh) return;
    const uint32_t n = (bh - r0 < rows ? bh - r0 : rows) * bw; // at most 2^26
    for (uint32_t k = lane; k < n; k += 64u) {
        const int32_t x = sx.first + (int32_t)(k % bw), y = sy.first + (int32_t)(r0 + k / bw); // inside the atlas: the spans are clamped
        float e1, e2;
        if (lm_covers(t, x, y, e1, e2)) atomicMin(owner + (size_t)y * (size_t)W + (size_t)x, tri);
    }
}

// One thread per texel: the owner's edge values again (lm_covers, the same instructions), the barycentrics, the point on the triangle's world
// vertices (write_prev's expression, rt_gbuffer_pixel.h) and the shading normal (gbuffer_pixel's expressions), then the texel's `repeats`
// entries: the point, the normal and the state of entry e = i * repeats + k. NULL outputs are not written.
__global__ void __launch_bounds__(kLmBlock) k_lm_texels(SceneDev S, const float* __restrict__ uv, const float* __restrict__ wv,
                                                         const uint32_t* __restrict__ owner, int32_t W, int32_t H, uint32_t repeats, uint32_t seed,
                                                         uint32_t* __restrict__ tri_out, float* __restrict__ pos_out, float* __restrict__ nrm_out,
                                                         uint32_t* __restrict__ state_out) {
    const uint32_t i = blockIdx.x * kLmBlock + threadIdx.x;
    if (i >= (uint32_t)W * (uint32_t)H) return;
    const uint32_t tri = owner[i];
    if (tri_out) tri_out[i] = tri;
    const float qnan = __uint_as_float(0x7FC00000u);
    f3 p = mk3(qnan, qnan, qnan), nrm = mk3(0.0f, 0.0f, 0.0f);
    if (tri != kNoTri) {
        const LmTri t = lm_tri(uv, tri, (float)W, (float)H);
        float e1, e2;
        (void)lm_covers(t, (int32_t)(i % (uint32_t)W), (int32_t)(i / (uint32_t)W), e1, e2);
        const float bx = e1 / t.area, by = e2 / t.area;
        const float w = (1.0f - bx) - by;
        const float* b = wv + 9 * (size_t)tri;
        p = mk3((b[0] * w + b[3] * bx) + b[6] * by, (b[1] * w + b[4] * bx) + b[7] * by, (b[2] * w + b[5] * bx) + b[8] * by);
        const ShadeRec& sr = S.shade[tri];
        const f3 n0 = mk3(sr.n0[0], sr.n0[1], sr.n0[2]), n1 = mk3(sr.n1[0], sr.n1[1], sr.n1[2]), n2 = mk3(sr.n2[0], sr.n2[1], sr.n2[2]);
        const uint32_t iw = sr.instance;
        const InstRec* inst = S.inst + (S.packed_mat ? (iw & kPackedInstMask) : iw);
        const f3 vn = normalize3((w * n0 + bx * n1) + by * n2);
        const float* nm = inst->normal_mat;
        const f3 g = mk3((nm[0] * vn.x + nm[3] * vn.y) + nm[6] * vn.z, (nm[1] * vn.x + nm[4] * vn.y) + nm[7] * vn.z,
                         (nm[2] * vn.x + nm[5] * vn.y) + nm[8] * vn.z);
        nrm = normalize3(g);
    }
    for (uint32_t k = 0; k < repeats; ++k) {
        const uint32_t e = i * repeats + k; // below 2^31 (rt_lightmap_create)
        if (pos_out) pos_out[3 * (size_t)e] = p.x, pos_out[3 * (size_t)e + 1] = p.y, pos_out[3 * (size_t)e + 2] = p.z;
        if (nrm_out) nrm_out[3 * (size_t)e] = nrm.x, nrm_out[3 * (size_t)e + 1] = nrm.y, nrm_out[3 * (size_t)e + 2] = nrm.z;
        if (state_out) {
            const uint32_t s = seed + (e + 1u) * 0x9E3779B9u;
            state_out[e] = s ? s : 0x9E3779B9u;
        }
    }
}

RT_DEV uint32_t lm_count(bool flag) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(flag)); }

// One wave per kLmWaveTexels texels, kLmLaneTexels per lane, 64 consecutive texels at a time: the mean of a texel's entries' radiances where
// it has an owner and no entry was rejected, alpha 1; else zeros. The statistics: covered and sampled texels as ballots, the rays of the
// entries not rejected as a wave sum; lane 0 adds them at the end. (One wave per 64 texels made 3 atomics per 64 texels on one cache line:
// 5.9 ms of an 80 ms bake at 4096 x 4096)
__global__ void __launch_bounds__(kLmStatBlock) k_lm_resolve(const uint32_t* __restrict__ owner, const float* __restrict__ rad,
                                                              const uint32_t* __restrict__ rays, uint32_t n, uint32_t repeats,
                                                              float4* __restrict__ out, rt_lightmap_stats* __restrict__ stats) {
    uint32_t n_cov = 0, n_smp = 0;
    unsigned long long traced = 0;
    for (uint32_t j = 0; j < kLmLaneTexels; ++j) {
        const uint32_t i = blockIdx.x * kLmWaveTexels + j * kLmStatBlock + threadIdx.x; // below 2^26 + kLmWaveTexels
        bool covered = false, sampled = false;
        if (i < n) {
            covered = owner[i] != kNoTri;
            bool rejected = false;
            for (uint32_t k = 0; k < repeats; ++k) {
                const uint32_t r = rays[i * repeats + k];
                if (r == 0xFFFFFFFFu) rejected = true;
                else traced += r;
            }
            sampled = covered && !rejected;
            float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (sampled) {
                float tx = 0.0f, ty = 0.0f, tz = 0.0f;
                for (uint32_t k = 0; k < repeats; ++k) {
                    const float* r = rad + 3 * (size_t)(i * repeats + k);
                    tx = tx + r[0], ty = ty + r[1], tz = tz + r[2];
                }
                const float d = (float)repeats;
                o = make_float4(tx / d, ty / d, tz / d, 1.0f);
            }
            out[i] = o;
        }
        n_cov += lm_count(covered), n_smp += lm_count(sampled);
    }
    for (int off = 32; off > 0; off >>= 1) traced += __shfl_xor(traced, off, 64);
    if (threadIdx.x == 0) {
        if (n_cov) atomicAdd(&stats->covered, n_cov);
        if (n_smp) atomicAdd(&stats->sampled, n_smp);
        if (traced) atomicAdd((unsigned long long*)&stats->rays, traced);
    }
}

// One dilation pass, the texels dealt to the waves as in k_lm_resolve: a texel with alpha 0 becomes the mean of its up to eight neighbours
// with alpha > 0, alpha 0.5; every other texel is copied. COUNT (the last pass): the texels with alpha 0.5 in the output.
template <bool COUNT>
__global__ void __launch_bounds__(kLmStatBlock) k_lm_dilate(const float4* __restrict__ in, int32_t W, int32_t H, float4* __restrict__ out,
                                                             rt_lightmap_stats* __restrict__ stats) {
    uint32_t n_filled = 0;
    for (uint32_t j = 0; j < kLmLaneTexels; ++j) {
        const uint32_t i = blockIdx.x * kLmWaveTexels + j * kLmStatBlock + threadIdx.x;
        bool filled = false;
        if (i < (uint32_t)W * (uint32_t)H) {
            const int32_t x = (int32_t)(i % (uint32_t)W), y = (int32_t)(i / (uint32_t)W);
            float4 c = in[i];
            if (c.w == 0.0f) {
                float sx = 0.0f, sy = 0.0f, sz = 0.0f;
                uint32_t n = 0;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    const int32_t qy = y + dy;
                    if (qy < 0 || qy >= H) continue;
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int32_t qx = x + dx;
                        if ((dx == 0 && dy == 0) || qx < 0 || qx >= W) continue;
                        const float4 q = in[qy * W + qx];
                        if (q.w > 0.0f) sx = sx + q.x, sy = sy + q.y, sz = sz + q.z, ++n;
                    }
                }
                if (n) {
                    const float d = (float)n;
                    c = make_float4(sx / d, sy / d, sz / d, 0.5f);
                }
            }
            out[i] = c;
            filled = c.w == 0.5f;
        }
        if (COUNT) n_filled += lm_count(filled);
    }
    if (COUNT && threadIdx.x == 0 && n_filled) atomicAdd(&stats->filled, n_filled);
}

} // namespace rt

namespace {

static_assert(sizeof(rt_lightmap_stats) == 24 && sizeof(rt_lightmap_params) == 24, "include/rt_mi355x.h states both sizes");

constexpr int32_t kMaxAtlas = 8192;
constexpr uint32_t kMaxDilate = 16;

// Waves per triangle for k_lm_owner: enough row bands that the largest clamped box is about kLmBandTexels texels per wave, no more than its
// rows, and no more waves in all than a launch grid holds. A sizing only: coverage does not depend on it.
uint32_t lm_bands(const float* uv, uint32_t n_tris, int32_t W, int32_t H) {
    uint64_t largest = 0;
    uint32_t rows = 1;
    for (uint32_t t = 0; t < n_tris; ++t) {
        const float* c = uv + 6 * (size_t)t;
        float lo[2], hi[2];
        bool fin = true;
        for (int a = 0; a < 2; ++a) {
            const float s = a ? (float)H : (float)W;
            const float v0 = c[a] * s, v1 = c[2 + a] * s, v2 = c[4 + a] * s;
            fin = fin && std::isfinite(v0) && std::isfinite(v1) && std::isfinite(v2);
            lo[a] = std::fmin(std::fmin(v0, v1), v2), hi[a] = std::fmax(std::fmax(v0, v1), v2);
        }
        if (!fin) continue;
        const LmSpan sx = lm_span(lo[0], hi[0], W), sy = lm_span(lo[1], hi[1], H);
        if (sx.last < sx.first || sy.last < sy.first) continue;
        const uint64_t bw = (uint64_t)(sx.last - sx.first + 1), bh = (uint64_t)(sy.last - sy.first + 1);
        if (bw * bh > largest) largest = bw * bh, rows = (uint32_t)bh;
    }
    uint64_t bands = (largest + kLmBandTexels - 1u) / kLmBandTexels;
    bands = std::min<uint64_t>(bands, rows);
    bands = std::min<uint64_t>(bands, kLmMaxWaves / std::max<uint32_t>(n_tris, 1u));
    return (uint32_t)std::max<uint64_t>(bands, 1u);
}

int check_params(const rt_lightmap_params* p) {
    if (!p) return fail(RT_ERR_INVALID, "null parameters");
    if (p->samples == 0) return fail(RT_ERR_INVALID, "samples must be at least 1");
    if (p->max_depth == 0) return fail(RT_ERR_INVALID, "max_depth must be at least 1");
    if (p->repeats == 0) return fail(RT_ERR_INVALID, "repeats must be at least 1");
    if (p->dilate > kMaxDilate) return fail(RT_ERR_INVALID, "dilate must be 0 .. 16");
    return RT_OK;
}

// the scene's world-space vertices as they are now: the scene's own on an updatable scene (an update may swap the pointer), else the copy
const float* world_vertices_of(const rt_lightmap* lm) { return lm->scene->upd ? lm->scene->upd->d_wv : lm->d_wv; }

// The owner plane and the texels' entries on st; the caller records the events. PRE: on the lightmap's device, st waited for ev_last.
int enqueue_texels(rt_lightmap* lm, uint32_t repeats, uint32_t seed, uint32_t* tri, float* pos, float* nrm, uint32_t* state, hipStream_t st) {
    const int32_t W = lm->width, H = lm->height;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    HIPCHK(hipMemsetAsync(lm->d_owner, 0xFF, (size_t)n * 4u, st));
    if (lm->n_tris) {
        const uint64_t waves = (uint64_t)lm->n_tris * lm->bands;
        hipLaunchKernelGGL(k_lm_owner, dim3((uint32_t)((waves + 3u) / 4u)), dim3(kLmBlock), 0, st, (const float*)lm->d_uv, lm->n_tris, W, H, lm->bands,
                           lm->d_owner);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lm_texels, dim3((n + kLmBlock - 1u) / kLmBlock), dim3(kLmBlock), 0, st, lm->scene->dev, (const float*)lm->d_uv,
                       world_vertices_of(lm), (const uint32_t*)lm->d_owner, W, H, repeats, seed, tri, pos, nrm, state);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

int begin_call(rt_lightmap* lm, hipStream_t st) {
    HIPCHK(hipSetDevice(lm->device));
    if (lm->recorded) HIPCHK(hipStreamWaitEvent(st, lm->ev_last, 0)); // the previous call (any stream) is done with the lightmap's buffers
    return RT_OK;
}

int end_call(rt_lightmap* lm, hipStream_t st) {
    HIPCHK(hipEventRecord(lm->ev_last, st));
    lm->recorded = true;
    return RT_OK;
}

// rt_lightmap_texels[_device]: the planes into tri / pos / nrm (device pointers, any may be null), and the scene's event behind the kernel
// that read its geometry. PRE: the arguments were checked
int texels_enqueue(rt_lightmap* lm, uint32_t* tri, float* pos, float* nrm, hipStream_t st) {
    if (const int rc = begin_call(lm, st)) return rc;
    hipEvent_t ev = nullptr;
    if (const int rc = scene_stream_event(lm->scene, st, &ev)) return rc;
    if (const int rc = enqueue_texels(lm, 1u, 0u, tri, pos, nrm, nullptr, st)) return rc;
    HIPCHK(hipEventRecord(ev, st));
    return end_call(lm, st);
}

// rt_lightmap_bake[_device]: the whole chain on st. out: the device plane the result goes to, or null (the host form: *result tells which
// of the lightmap's own planes holds it). PRE: the arguments were checked
int bake_enqueue(rt_lightmap* lm, const rt_lightmap_params* p, float4* out, rt_lightmap_stats* stats, hipStream_t st, float4** result) {
    if (const int rc = begin_call(lm, st)) return rc;
    const int32_t W = lm->width, H = lm->height;
    const uint32_t n = (uint32_t)W * (uint32_t)H, R = p->repeats;
    if (const int rc = enqueue_texels(lm, R, p->seed, nullptr, lm->d_pos, lm->d_nrm, lm->d_state, st)) return rc;
    rt_gather_query q{};
    q.n = n * R, q.max_depth = p->max_depth, q.samples = p->samples, q.rr_start = p->rr_start;
    q.pos = lm->d_pos, q.normal = lm->d_nrm, q.rng = lm->d_state, q.rng_out = nullptr, q.radiance = lm->d_rad, q.rays = lm->d_rays;
    if (const int rc = rt_gather_paths_device(lm->scene, &q, st)) return rc; // records the scene's event for st behind k_lm_texels too
    HIPCHK(hipSetDevice(lm->device));
    rt_lightmap_stats* d_stats = stats ? stats : lm->d_stats;
    HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(rt_lightmap_stats), st));
    float4* last = out ? out : lm->d_plane[p->dilate & 1u];
    const dim3 grid((n + kLmWaveTexels - 1u) / kLmWaveTexels), block(kLmStatBlock);
    hipLaunchKernelGGL(k_lm_resolve, grid, block, 0, st, (const uint32_t*)lm->d_owner, (const float*)lm->d_rad, (const uint32_t*)lm->d_rays, n, R,
                       p->dilate ? lm->d_plane[0] : last, d_stats);
    HIPCHK(hipGetLastError());
    for (uint32_t j = 0; j < p->dilate; ++j) {
        const float4* src = lm->d_plane[j & 1u];
        if (j + 1 == p->dilate) hipLaunchKernelGGL(k_lm_dilate<true>, grid, block, 0, st, src, W, H, last, d_stats);
        else hipLaunchKernelGGL(k_lm_dilate<false>, grid, block, 0, st, src, W, H, lm->d_plane[(j + 1u) & 1u], d_stats);
        HIPCHK(hipGetLastError());
    }
    if (result) *result = last;
    return end_call(lm, st);
}

int bake_check(const rt_lightmap* lm, const rt_lightmap_params* p, const void* out) {
    if (const int rc = check_params(p)) return rc;
    if (!lm || !out) return fail(RT_ERR_INVALID, "null argument");
    if (p->repeats > lm->max_repeats) return fail(RT_ERR_INVALID, "repeats exceeds the max_repeats the lightmap was created with");
    return RT_OK;
}

} // namespace

extern "C" {

int rt_lightmap_create(rt_scene* s, int32_t width, int32_t height, uint32_t max_repeats, const float* lm_uv, rt_lightmap** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (!s) return fail(RT_ERR_INVALID, "null scene");
    if (width < 1 || width > kMaxAtlas || height < 1 || height > kMaxAtlas) return fail(RT_ERR_INVALID, "width and height must be 1 .. 8192");
    if (max_repeats == 0) return fail(RT_ERR_INVALID, "max_repeats must be at least 1");
    if ((uint64_t)width * (uint64_t)height * max_repeats > 0x7fffffffull)
        return fail(RT_ERR_INVALID, "too many entries (W x H x max_repeats must stay below 2^31)");
    const uint32_t T = (uint32_t)(s->hs.wverts.size() / 9);
    if (T && !lm_uv) return fail(RT_ERR_INVALID, "null lm_uv");
    if (s->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    HIPCHK(hipSetDevice(s->device));
    return no_throw([&]() -> int {
        rt_lightmap* lm = new rt_lightmap;
        lm->scene = s, lm->device = s->device, lm->width = width, lm->height = height, lm->max_repeats = max_repeats, lm->n_tris = T;
        lm->bands = lm_bands(lm_uv, T, width, height);
        const size_t n = (size_t)width * (size_t)height, e = n * max_repeats;
        const bool copy_wv = !s->upd;
        if (hipMalloc((void**)&lm->d_uv, std::max<size_t>(T, 1) * 24u) != hipSuccess ||
            (copy_wv && hipMalloc((void**)&lm->d_wv, std::max<size_t>(T, 1) * 36u) != hipSuccess) ||
            hipMalloc((void**)&lm->d_owner, n * 4u) != hipSuccess || hipMalloc((void**)&lm->d_pos, e * 12u) != hipSuccess ||
            hipMalloc((void**)&lm->d_nrm, e * 12u) != hipSuccess || hipMalloc((void**)&lm->d_state, e * 4u) != hipSuccess ||
            hipMalloc((void**)&lm->d_rad, e * 12u) != hipSuccess || hipMalloc((void**)&lm->d_rays, e * 4u) != hipSuccess ||
            hipMalloc((void**)&lm->d_plane[0], n * 16u) != hipSuccess || hipMalloc((void**)&lm->d_plane[1], n * 16u) != hipSuccess ||
            hipMalloc((void**)&lm->d_stats, sizeof(rt_lightmap_stats)) != hipSuccess) {
            rt_lightmap_destroy(lm);
            return fail(RT_ERR_OOM, "hipMalloc of the lightmap's buffers failed");
        }
        if (T && (hipMemcpy(lm->d_uv, lm_uv, (size_t)T * 24u, hipMemcpyHostToDevice) != hipSuccess ||
                  (copy_wv && hipMemcpy(lm->d_wv, s->hs.wverts.data(), (size_t)T * 36u, hipMemcpyHostToDevice) != hipSuccess))) {
            rt_lightmap_destroy(lm);
            return fail(RT_ERR_HIP, "hipMemcpy of the lightmap's UVs and vertices failed");
        }
        if (hipStreamCreateWithFlags(&lm->stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&lm->ev_last, hipEventDisableTiming) != hipSuccess) {
            rt_lightmap_destroy(lm);
            return fail(RT_ERR_HIP, "hipStreamCreate / hipEventCreate failed");
        }
        *out = lm;
        return (int)RT_OK;
    });
}

void rt_lightmap_destroy(rt_lightmap* lm) {
    if (!lm) return;
    if (lm->device >= 0 && hipSetDevice(lm->device) == hipSuccess) {
        if (lm->recorded) (void)hipEventSynchronize(lm->ev_last);
        for (void* p : {(void*)lm->d_uv, (void*)lm->d_wv, (void*)lm->d_owner, (void*)lm->d_pos, (void*)lm->d_nrm, (void*)lm->d_state, (void*)lm->d_rad,
                        (void*)lm->d_rays, (void*)lm->d_plane[0], (void*)lm->d_plane[1], (void*)lm->d_stats})
            (void)hipFree(p);
        if (lm->ev_last) (void)hipEventDestroy(lm->ev_last);
        if (lm->stream) (void)hipStreamDestroy(lm->stream);
    }
    delete lm;
}

int rt_lightmap_texels(rt_lightmap* lm, uint32_t* tri, float* pos, float* normal) {
    if (!lm) return fail(RT_ERR_INVALID, "null argument");
    if (!tri && !pos && !normal) return fail(RT_ERR_INVALID, "tri, pos and normal are all null");
    hipStream_t st = lm->stream;
    if (const int rc = texels_enqueue(lm, nullptr, lm->d_pos, lm->d_nrm, st)) return rc;
    const size_t n = (size_t)lm->width * (size_t)lm->height;
    if (tri) HIPCHK(hipMemcpyAsync(tri, lm->d_owner, n * 4u, hipMemcpyDeviceToHost, st));
    if (pos) HIPCHK(hipMemcpyAsync(pos, lm->d_pos, n * 12u, hipMemcpyDeviceToHost, st));
    if (normal) HIPCHK(hipMemcpyAsync(normal, lm->d_nrm, n * 12u, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_lightmap_texels_device(rt_lightmap* lm, void* d_tri, void* d_pos, void* d_normal, void* stream) {
    if (!lm) return fail(RT_ERR_INVALID, "null argument");
    if (!d_tri && !d_pos && !d_normal) return fail(RT_ERR_INVALID, "tri, pos and normal are all null");
    return texels_enqueue(lm, (uint32_t*)d_tri, (float*)d_pos, (float*)d_normal, (hipStream_t)stream);
}

int rt_lightmap_bake(rt_lightmap* lm, const rt_lightmap_params* p, float* out_rgba, rt_lightmap_stats* stats) {
    if (const int rc = bake_check(lm, p, out_rgba)) return rc;
    hipStream_t st = lm->stream;
    float4* result = nullptr;
    if (const int rc = bake_enqueue(lm, p, nullptr, nullptr, st, &result)) return rc;
    HIPCHK(hipMemcpyAsync(out_rgba, result, (size_t)lm->width * (size_t)lm->height * 16u, hipMemcpyDeviceToHost, st));
    if (stats) HIPCHK(hipMemcpyAsync(stats, lm->d_stats, sizeof(rt_lightmap_stats), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_lightmap_bake_device(rt_lightmap* lm, const rt_lightmap_params* p, void* d_out_rgba, void* d_stats, void* stream) {
    if (const int rc = bake_check(lm, p, d_out_rgba)) return rc;
    return bake_enqueue(lm, p, (float4*)d_out_rgba, (rt_lightmap_stats*)d_stats, (hipStream_t)stream, nullptr);
}

} // extern "C"
