// rt_lightmap.hip — lightmap baking: rt_lightmap_create[_ex] / _destroy, rt_lightmap_texels[_device], rt_lightmap_bake[_device], and for a
// lightmap created with RT_LIGHTMAP_FILTER rt_lightmap_bake_filtered[_device] and rt_lightmap_filter[_device], and their kernels.
// The atlas-side half of a lightmap bake around one gather query (rt_path_gather.hip, called through its public entry point): which triangle
// owns a texel (k_lm_owner), where the texel lies on it and with which shading normal, and the states of its entries (k_lm_texels), the mean
// of the entries' radiances (k_lm_resolve<false>) and the filling of the gutters (k_lm_dilate). The arithmetic is the contract stated at
// rt_lightmap_bake in include/rt_mi355x.h; the numpy model that pins it bit for bit is tests/test_lightmap.py. No traversal, no LDS, no
// float atomics in this unit: the owner plane is an integer minimum, the statistics are ballots and integer sums.
// The filter (the contract's steps 5a and 5b, the model tests/test_lightmap_filter.py): k_lm_resolve<true> is the same text with the variance of
// the texel's mean in .w and the two guide planes, k_lm_atrous one a-trous iteration in texel space, one launch per iteration, the kernel
// boundary the only hand-off, in rt_image_op.h's 64 x 4 tile shape. Its tap loop is this unit's own: the mask is a plane (.w of the position
// guide), the variance prefilter is renormalised over the mask, the values are linear and there is no albedo. The helpers it is made of
// (exp_m, dot_diff, luminance, kTapH, kPreK, coefficient) are rt_atrous_pixel.h's and its includes', read from there.
#include "rt_internal.h"
#include "rt_device.h"
#include "rt_atrous_pixel.h"

struct rt_lightmap : CallBracket { // the host forms run on its stream
    rt_scene* scene = nullptr;
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
    uint32_t flags = 0;              // RT_LIGHTMAP_*
    // RT_LIGHTMAP_FILTER: the guide planes (position with the mask in .w, normal) and the host forms' staging
    float4* d_gpos = nullptr;
    float4* d_gnrm = nullptr;
    float4* d_host_rgba = nullptr;
    float* d_host_var_in = nullptr;
    float* d_host_var_out = nullptr;
    rt_lightmap_stats* d_stats = nullptr;
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
// it has an owner and no entry was rejected; else zeros. The statistics: covered and sampled texels as ballots, the rays of the entries not
// rejected as a wave sum; lane 0 adds them at the end. (One wave per 64 texels made 3 atomics per 64 texels on one cache line: 5.9 ms of an
// 80 ms bake at 4096 x 4096)
// VAR = false (rt_lightmap_bake): .w of the output is alpha, 1 where sampled; pos, nrm, gpos and gnrm are not looked at.
// VAR = true (the filter's step 5a): .w is the variance of the texel's mean luminance (0 where not sampled, and for one repeat); the mask goes
// to .w of the position guide, 1 where sampled. The guides are the texel's first entry's.
template <bool VAR>
__global__ void __launch_bounds__(kLmStatBlock) k_lm_resolve(const uint32_t* __restrict__ owner, const float* __restrict__ rad,
                                                              const uint32_t* __restrict__ rays, uint32_t n, uint32_t repeats,
                                                              float4* __restrict__ out, rt_lightmap_stats* __restrict__ stats,
                                                              const float* __restrict__ pos, const float* __restrict__ nrm,
                                                              float4* __restrict__ gpos, float4* __restrict__ gnrm) {
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
                const float d = (float)repeats;
                float tx = 0.0f, ty = 0.0f, tz = 0.0f, tl = 0.0f;
                for (uint32_t k = 0; k < repeats; ++k) {
                    const float* r = rad + 3 * (size_t)(i * repeats + k);
                    tx = tx + r[0], ty = ty + r[1], tz = tz + r[2];
                    if (VAR) tl = tl + luminance(make_float4(r[0], r[1], r[2], 0.0f));
                }
                float w = 1.0f;
                if (VAR) {
                    w = 0.0f;
                    if (repeats > 1) {
                        const float m = tl / d;
                        float s = 0.0f;
                        for (uint32_t k = 0; k < repeats; ++k) {
                            const float* r = rad + 3 * (size_t)(i * repeats + k);
                            const float dl = luminance(make_float4(r[0], r[1], r[2], 0.0f)) - m;
                            s = s + dl * dl;
                        }
                        w = s / (d * (float)(repeats - 1u));
                    }
                }
                o = make_float4(tx / d, ty / d, tz / d, w);
            }
            out[i] = o;
            if (VAR) {
                const float* p = pos + 3 * (size_t)(i * repeats);
                const float* q = nrm + 3 * (size_t)(i * repeats);
                gpos[i] = make_float4(p[0], p[1], p[2], sampled ? 1.0f : 0.0f);
                gnrm[i] = make_float4(q[0], q[1], q[2], 0.0f);
            }
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

// ---- the filter (RT_LIGHTMAP_FILTER) ---------------------------------------------------------------------------------------------------------
// rt_lightmap_filter's planes from the caller's: one thread per texel. In M (alpha 1, an owner, six finite guide floats): rgb with the variance
// in .w (0 without a variance plane); else zeros. The guides are k_lm_texels' for one repeat. `out` may be `rgba`: a thread reads its texel first.
__global__ void __launch_bounds__(kLmBlock) k_lm_filter_in(const float4* rgba, const float* __restrict__ var, const uint32_t* __restrict__ owner,
                                                            const float* __restrict__ pos, const float* __restrict__ nrm, uint32_t n, float4* out,
                                                            float4* __restrict__ gpos, float4* __restrict__ gnrm) {
    const uint32_t i = blockIdx.x * kLmBlock + threadIdx.x;
    if (i >= n) return;
    const float4 c = rgba[i];
    const float* p = pos + 3 * (size_t)i;
    const float* q = nrm + 3 * (size_t)i;
    const bool in = c.w == 1.0f && owner[i] != kNoTri && __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]) &&
                    __builtin_isfinite(q[0]) && __builtin_isfinite(q[1]) && __builtin_isfinite(q[2]);
    out[i] = in ? make_float4(c.x, c.y, c.z, var ? var[i] : 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    gpos[i] = make_float4(p[0], p[1], p[2], in ? 1.0f : 0.0f);
    gnrm[i] = make_float4(q[0], q[1], q[2], 0.0f);
}

// What leaves the filter: alpha in .w again (1 on M, where the plane's .w is the variance; outside M the plane is zeros) and the variance plane
// (may be null). The whole filter for iterations = 0, and the last lines of k_lm_atrous<true>.
RT_DEV void lm_filter_out(uint32_t p, float4 c, bool in, float4* __restrict__ out, float* __restrict__ out_var) {
    out[p] = make_float4(c.x, c.y, c.z, in ? 1.0f : 0.0f);
    if (out_var) out_var[p] = c.w;
}
__global__ void __launch_bounds__(kLmBlock) k_lm_filter_copy(const float4* __restrict__ in, const float4* __restrict__ gpos, uint32_t n,
                                                              float4* __restrict__ out, float* __restrict__ out_var) {
    const uint32_t i = blockIdx.x * kLmBlock + threadIdx.x;
    if (i < n) lm_filter_out(i, in[i], gpos[i].w != 0.0f, out, out_var);
}

// One iteration of step 5b with step `step` at the thread's texel (tile_pixel: a wave is one row of 64 consecutive texels). in: rgb with the
// variance in .w, zeros outside M; gpos: position, .w the mask; gnrm: normal, not read where kn is 0. use_l: the luminance term is on (sigma_l
// finite), scaled by the 3 x 3 prefilter of the variance at p over the taps in M. LAST: alpha instead of the variance in out.w, the variance to
// out_var (may be null). A texel outside M writes zeros and leaves, so a wave whose row holds none ends at its first branch: the exit of an
// empty tile needs no ballot of its own. EARLY = false (the developer build's RT_LM_FILTER_NO_EARLY_EXIT, for the probe's comparison): such
// a texel walks its taps like the others and writes its zeros at the end.
template <bool LAST, bool EARLY = true>
__global__ void __launch_bounds__(256) k_lm_atrous(const float4* __restrict__ in, const float4* __restrict__ gpos, const float4* __restrict__ gnrm,
                                                    int32_t W, int32_t H, int32_t step, int32_t use_l, float sigma_l, float kn, float kx,
                                                    float4* __restrict__ out, float* __restrict__ out_var) {
    int32_t x, y;
    if (!tile_pixel(W, H, &x, &y)) return;
    const int32_t p = y * W + x;
    const float4 Pp = gpos[p];
    if (EARLY && Pp.w == 0.0f) {
        out[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (LAST && out_var) out_var[p] = 0.0f;
        return;
    }
    const float4 Lp = in[p];
    const float4 Np = kn != 0.0f ? gnrm[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float lp = luminance(Lp);
    float kl = 0.0f;
    if (use_l) {
        float g = 0.0f, ks = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int32_t qy = y + dy;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int32_t qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const int32_t q = qy * W + qx;
                if (gpos[q].w == 0.0f) continue;
                const float k = kPreK[dy + 1] * kPreK[dx + 1];
                g = g + k * in[q].w;
                ks = ks + k;
            }
        }
        kl = 1.0f / (sigma_l * __builtin_sqrtf(g / ks) + kLumEps);
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int32_t qy = y + step * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int32_t qx = x + step * dx;
            if (qx < 0 || qx >= W) continue;
            const int32_t q = qy * W + qx;
            const float4 Pq = gpos[q];
            if (Pq.w == 0.0f) continue;
            const float4 Lq = in[q];
            float E = 0.0f;
            if (use_l) E = E + __builtin_fabsf(lp - luminance(Lq)) * kl;
            if (kn != 0.0f) E = E + dot_diff(Np, gnrm[q]) * kn;
            if (kx != 0.0f) E = E + dot_diff(Pp, Pq) * kx;
            const float w = (kTapH[dy + 2] * kTapH[dx + 2]) * exp_m(-E);
            sx = sx + w * Lq.x, sy = sy + w * Lq.y, sz = sz + w * Lq.z;
            wsum = wsum + w;
            sv = sv + (w * w) * Lq.w;
        }
    }
    float4 c = make_float4(sx / wsum, sy / wsum, sz / wsum, sv / (wsum * wsum));
    if (!EARLY && Pp.w == 0.0f) c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (LAST) lm_filter_out((uint32_t)p, c, Pp.w != 0.0f, out, out_var);
    else out[p] = c;
}

} // namespace rt

namespace {

static_assert(sizeof(rt_lightmap_stats) == 24 && sizeof(rt_lightmap_params) == 24 && sizeof(rt_lightmap_filter_params) == 16,
              "include/rt_mi355x.h states the sizes");

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
const float* world_vertices_of(const rt_lightmap* lm) { return lm->scene->upd ? lm->scene->upd->d_wv.get() : lm->d_wv; }

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

// A call that reads the scene's geometry without a gather: the owner plane and the planes of one entry per texel into tri / pos / nrm (device
// pointers, any may be null), and the scene's event for st behind the kernel that read the geometry. PRE: the call's bracket is open
int enqueue_geometry(rt_lightmap* lm, uint32_t* tri, float* pos, float* nrm, hipStream_t st) {
    hipEvent_t ev = nullptr;
    if (const int rc = scene_stream_event(lm->scene, st, &ev)) return rc;
    if (const int rc = enqueue_texels(lm, 1u, 0u, tri, pos, nrm, nullptr, st)) return rc;
    HIPCHK(hipEventRecord(ev, st));
    return RT_OK;
}

// rt_lightmap_texels[_device]. PRE: the arguments were checked
int texels_enqueue(rt_lightmap* lm, uint32_t* tri, float* pos, float* nrm, hipStream_t st) {
    if (const int rc = begin_call(lm, st)) return rc;
    if (const int rc = enqueue_geometry(lm, tri, pos, nrm, st)) return rc;
    return end_call(lm, st);
}

// ---- the checks (the entry points judge the parameters first: they need no lightmap) ------------------------------------------------------
int check_filter_params(const rt_lightmap_filter_params* f) {
    if (f->iterations > kMaxIterations) return fail(RT_ERR_INVALID, "iterations must be 0 .. 10");
    const float s[3] = {f->sigma_luminance, f->sigma_normal, f->sigma_position};
    for (float v : s)
        if (!(v >= kMinSigma)) return fail(RT_ERR_INVALID, "every sigma must be at least 1e-6 (+inf ignores its guide); NaN is refused");
    return RT_OK;
}

int check_filter_flag(const rt_lightmap* lm) {
    if (!(lm->flags & RT_LIGHTMAP_FILTER)) return fail(RT_ERR_INVALID, "the lightmap was created without RT_LIGHTMAP_FILTER (rt_lightmap_create_ex)");
    return RT_OK;
}

// The filter stage of a bake (rt_lightmap_bake_filtered[_device]); rt_lightmap_bake[_device] has none. f null: no filter, that call's identity,
// which still keeps the variance and the guides. out_var: a device plane or null
struct FilterStage {
    const rt_lightmap_filter_params* f;
    float* out_var;
};

// fs null: rt_lightmap_bake[_device]
int bake_check(const rt_lightmap* lm, const rt_lightmap_params* p, const FilterStage* fs, const void* out) {
    if (const int rc = check_params(p)) return rc;
    if (fs && fs->f) {
        if (const int rc = check_filter_params(fs->f)) return rc;
        if (fs->f->iterations > 0 && !std::isinf(fs->f->sigma_luminance) && p->repeats < 2)
            return fail(RT_ERR_INVALID, "a finite sigma_luminance needs repeats >= 2: one entry per texel has no noise estimate");
    }
    if (!lm || !out) return fail(RT_ERR_INVALID, "null argument");
    if (fs)
        if (const int rc = check_filter_flag(lm)) return rc;
    if (p->repeats > lm->max_repeats) return fail(RT_ERR_INVALID, "repeats exceeds the max_repeats the lightmap was created with");
    return RT_OK;
}

int filter_check(const rt_lightmap* lm, const rt_lightmap_filter_params* f, const void* rgba, const void* var, const void* out) {
    if (!f) return fail(RT_ERR_INVALID, "null parameters");
    if (const int rc = check_filter_params(f)) return rc;
    if (!var && !std::isinf(f->sigma_luminance)) return fail(RT_ERR_INVALID, "variance may be null only with sigma_luminance = +inf");
    if (!lm || !rgba || !out) return fail(RT_ERR_INVALID, "null argument");
    return check_filter_flag(lm);
}

// ---- the filter (RT_LIGHTMAP_FILTER) ---------------------------------------------------------------------------------------------------------
// the plane the filter's result lies in where it stays in the lightmap: the last launch reads d_plane[(iters - 1) & 1], or d_plane[0] without one
uint32_t filtered_plane(const rt_lightmap_filter_params* f) { return f && f->iterations ? (f->iterations & 1u) : 1u; }

// Step 5b on st: the iterations from d_plane[0] (rgb, variance) and the guide planes, ping-pong through the two planes, the last into dst with
// alpha and into out_var (may be null). dst is none of the lightmap's planes, or d_plane[filtered_plane(f)]. PRE: the call's bracket is open
int enqueue_filter(rt_lightmap* lm, const rt_lightmap_filter_params* f, float4* dst, float* out_var, hipStream_t st) {
    const int32_t W = lm->width, H = lm->height;
    const uint32_t n = (uint32_t)W * (uint32_t)H, iters = f ? f->iterations : 0u;
    if (iters == 0) {
        hipLaunchKernelGGL(k_lm_filter_copy, dim3((n + kLmBlock - 1u) / kLmBlock), dim3(kLmBlock), 0, st, (const float4*)lm->d_plane[0],
                           (const float4*)lm->d_gpos, n, dst, out_var);
        HIPCHK(hipGetLastError());
        return RT_OK;
    }
    const int32_t use_l = std::isinf(f->sigma_luminance) ? 0 : 1;
    const float kn = coefficient(f->sigma_normal), kx = coefficient(f->sigma_position);
    auto last_kernel = k_lm_atrous<true>;
    auto other_kernel = k_lm_atrous<false>;
#ifdef RT_DEVELOPER_KNOBS
    if (dev_knob("RT_LM_FILTER_NO_EARLY_EXIT")) last_kernel = k_lm_atrous<true, false>, other_kernel = k_lm_atrous<false, false>;
#endif
    for (uint32_t i = 0; i < iters; ++i) {
        const bool last = i + 1 == iters;
        hipLaunchKernelGGL(last ? last_kernel : other_kernel, tile_grid(W, H), tile_block(), 0, st, (const float4*)lm->d_plane[i & 1u],
                           (const float4*)lm->d_gpos, (const float4*)lm->d_gnrm, W, H, 1 << i, use_l, f->sigma_luminance,
                           std::ldexp(kn, -2 * (int)i), kx, last ? dst : lm->d_plane[(i + 1u) & 1u], last ? out_var : (float*)nullptr);
        HIPCHK(hipGetLastError());
    }
    return RT_OK;
}

// rt_lightmap_bake[_device] (fs null) and rt_lightmap_bake_filtered[_device]: the whole chain on st. The resolve, with a filter stage the one that
// keeps the variance and the guides and behind it the filter, leaves its plane in d_plane[first]; the dilation ping-pongs on from there. out: the
// device plane the result goes to, or null (the host form: *result tells which of the lightmap's own planes holds it). PRE: the arguments were checked
int bake_enqueue(rt_lightmap* lm, const rt_lightmap_params* p, const FilterStage* fs, float4* out, rt_lightmap_stats* stats, hipStream_t st,
                 float4** result) {
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
    const uint32_t first = fs ? filtered_plane(fs->f) : 0u, dilate = p->dilate;
    float4* last = out ? out : lm->d_plane[(first + dilate) & 1u];
    float4* undilated = dilate ? lm->d_plane[first] : last;
    const dim3 grid((n + kLmWaveTexels - 1u) / kLmWaveTexels), block(kLmStatBlock);
    hipLaunchKernelGGL(fs ? k_lm_resolve<true> : k_lm_resolve<false>, grid, block, 0, st, (const uint32_t*)lm->d_owner, (const float*)lm->d_rad,
                       (const uint32_t*)lm->d_rays, n, R, fs ? lm->d_plane[0] : undilated, d_stats, (const float*)lm->d_pos, (const float*)lm->d_nrm,
                       lm->d_gpos, lm->d_gnrm);
    HIPCHK(hipGetLastError());
    if (fs)
        if (const int rc = enqueue_filter(lm, fs->f, undilated, fs->out_var, st)) return rc;
    for (uint32_t j = 0; j < dilate; ++j) {
        const float4* src = lm->d_plane[(first + j) & 1u];
        if (j + 1 == dilate) hipLaunchKernelGGL(k_lm_dilate<true>, grid, block, 0, st, src, W, H, last, d_stats);
        else hipLaunchKernelGGL(k_lm_dilate<false>, grid, block, 0, st, src, W, H, lm->d_plane[(first + j + 1u) & 1u], d_stats);
        HIPCHK(hipGetLastError());
    }
    if (result) *result = last;
    return end_call(lm, st);
}

// rt_lightmap_filter[_device] behind the wait: the lightmap's guides as they are now, the caller's planes cut to the mask, the filter, the call's
// end. All pointers are device pointers; var and out_var may be null. PRE: the arguments were checked and the call's bracket is open (the host
// form has staged its arguments in it)
int filter_enqueue(rt_lightmap* lm, const rt_lightmap_filter_params* f, const float4* rgba, const float* var, float4* out, float* out_var,
                   hipStream_t st) {
    if (const int rc = enqueue_geometry(lm, nullptr, lm->d_pos, lm->d_nrm, st)) return rc;
    const uint32_t n = (uint32_t)lm->width * (uint32_t)lm->height;
    hipLaunchKernelGGL(k_lm_filter_in, dim3((n + kLmBlock - 1u) / kLmBlock), dim3(kLmBlock), 0, st, rgba, var, (const uint32_t*)lm->d_owner,
                       (const float*)lm->d_pos, (const float*)lm->d_nrm, n, lm->d_plane[0], lm->d_gpos, lm->d_gnrm);
    HIPCHK(hipGetLastError());
    if (const int rc = enqueue_filter(lm, f, out, out_var, st)) return rc;
    return end_call(lm, st);
}

// The end of the host forms, behind the call on the lightmap's stream: the rgba plane, the variance plane from its staging and the statistics
// (each of the last two where its pointer is not null) to the host, and the stream has run dry
int host_results(rt_lightmap* lm, const float4* d_rgba, float* out_rgba, float* out_variance, rt_lightmap_stats* stats) {
    hipStream_t st = lm->stream;
    const size_t n = (size_t)lm->width * (size_t)lm->height;
    HIPCHK(hipMemcpyAsync(out_rgba, d_rgba, n * 16u, hipMemcpyDeviceToHost, st));
    if (out_variance) HIPCHK(hipMemcpyAsync(out_variance, lm->d_host_var_out, n * 4u, hipMemcpyDeviceToHost, st));
    if (stats) HIPCHK(hipMemcpyAsync(stats, lm->d_stats, sizeof(rt_lightmap_stats), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_lightmap_create(rt_scene* s, int32_t width, int32_t height, uint32_t max_repeats, const float* lm_uv, rt_lightmap** out) {
    return rt_lightmap_create_ex(s, width, height, max_repeats, lm_uv, 0u, out);
}

int rt_lightmap_create_ex(rt_scene* s, int32_t width, int32_t height, uint32_t max_repeats, const float* lm_uv, uint32_t flags, rt_lightmap** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (!s) return fail(RT_ERR_INVALID, "null scene");
    if (flags & ~RT_LIGHTMAP_FILTER) return fail(RT_ERR_INVALID, "unknown lightmap flag");
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
        lm->bands = lm_bands(lm_uv, T, width, height), lm->flags = flags;
        const size_t n = (size_t)width * (size_t)height, e = n * max_repeats;
        const bool copy_wv = !s->upd, filter = (flags & RT_LIGHTMAP_FILTER) != 0;
        if (hipMalloc((void**)&lm->d_uv, std::max<size_t>(T, 1) * 24u) != hipSuccess ||
            (copy_wv && hipMalloc((void**)&lm->d_wv, std::max<size_t>(T, 1) * 36u) != hipSuccess) ||
            hipMalloc((void**)&lm->d_owner, n * 4u) != hipSuccess || hipMalloc((void**)&lm->d_pos, e * 12u) != hipSuccess ||
            hipMalloc((void**)&lm->d_nrm, e * 12u) != hipSuccess || hipMalloc((void**)&lm->d_state, e * 4u) != hipSuccess ||
            hipMalloc((void**)&lm->d_rad, e * 12u) != hipSuccess || hipMalloc((void**)&lm->d_rays, e * 4u) != hipSuccess ||
            hipMalloc((void**)&lm->d_plane[0], n * 16u) != hipSuccess || hipMalloc((void**)&lm->d_plane[1], n * 16u) != hipSuccess ||
            hipMalloc((void**)&lm->d_stats, sizeof(rt_lightmap_stats)) != hipSuccess ||
            (filter && (hipMalloc((void**)&lm->d_gpos, n * 16u) != hipSuccess || hipMalloc((void**)&lm->d_gnrm, n * 16u) != hipSuccess ||
                        hipMalloc((void**)&lm->d_host_rgba, n * 16u) != hipSuccess || hipMalloc((void**)&lm->d_host_var_in, n * 4u) != hipSuccess ||
                        hipMalloc((void**)&lm->d_host_var_out, n * 4u) != hipSuccess))) {
            rt_lightmap_destroy(lm);
            return fail(RT_ERR_OOM, "hipMalloc of the lightmap's buffers failed");
        }
        if (T && (hipMemcpy(lm->d_uv, lm_uv, (size_t)T * 24u, hipMemcpyHostToDevice) != hipSuccess ||
                  (copy_wv && hipMemcpy(lm->d_wv, s->hs.wverts.data(), (size_t)T * 36u, hipMemcpyHostToDevice) != hipSuccess))) {
            rt_lightmap_destroy(lm);
            return fail(RT_ERR_HIP, "hipMemcpy of the lightmap's UVs and vertices failed");
        }
        if (const int rc = bracket_open(lm)) {
            rt_lightmap_destroy(lm);
            return rc;
        }
        *out = lm;
        return (int)RT_OK;
    });
}

void rt_lightmap_destroy(rt_lightmap* lm) {
    if (!lm) return;
    if (bracket_close(lm))
        for (void* p : {(void*)lm->d_uv, (void*)lm->d_wv, (void*)lm->d_owner, (void*)lm->d_pos, (void*)lm->d_nrm, (void*)lm->d_state, (void*)lm->d_rad,
                        (void*)lm->d_rays, (void*)lm->d_plane[0], (void*)lm->d_plane[1], (void*)lm->d_stats, (void*)lm->d_gpos, (void*)lm->d_gnrm,
                        (void*)lm->d_host_rgba, (void*)lm->d_host_var_in, (void*)lm->d_host_var_out})
            (void)hipFree(p);
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
    if (const int rc = bake_check(lm, p, nullptr, out_rgba)) return rc;
    float4* result = nullptr;
    if (const int rc = bake_enqueue(lm, p, nullptr, nullptr, nullptr, lm->stream, &result)) return rc;
    return host_results(lm, result, out_rgba, nullptr, stats);
}

int rt_lightmap_bake_device(rt_lightmap* lm, const rt_lightmap_params* p, void* d_out_rgba, void* d_stats, void* stream) {
    if (const int rc = bake_check(lm, p, nullptr, d_out_rgba)) return rc;
    return bake_enqueue(lm, p, nullptr, (float4*)d_out_rgba, (rt_lightmap_stats*)d_stats, (hipStream_t)stream, nullptr);
}

int rt_lightmap_bake_filtered(rt_lightmap* lm, const rt_lightmap_params* p, const rt_lightmap_filter_params* f, float* out_rgba, float* out_variance,
                              rt_lightmap_stats* stats) {
    FilterStage fs{f, nullptr};
    if (const int rc = bake_check(lm, p, &fs, out_rgba)) return rc;
    fs.out_var = out_variance ? lm->d_host_var_out : nullptr;
    float4* result = nullptr;
    if (const int rc = bake_enqueue(lm, p, &fs, nullptr, nullptr, lm->stream, &result)) return rc;
    return host_results(lm, result, out_rgba, out_variance, stats);
}

int rt_lightmap_bake_filtered_device(rt_lightmap* lm, const rt_lightmap_params* p, const rt_lightmap_filter_params* f, void* d_out_rgba,
                                     void* d_out_variance, void* d_stats, void* stream) {
    const FilterStage fs{f, (float*)d_out_variance};
    if (const int rc = bake_check(lm, p, &fs, d_out_rgba)) return rc;
    return bake_enqueue(lm, p, &fs, (float4*)d_out_rgba, (rt_lightmap_stats*)d_stats, (hipStream_t)stream, nullptr);
}

int rt_lightmap_filter(rt_lightmap* lm, const rt_lightmap_filter_params* f, const float* rgba, const float* variance, float* out_rgba,
                       float* out_variance) {
    if (const int rc = filter_check(lm, f, rgba, variance, out_rgba)) return rc;
    hipStream_t st = lm->stream;
    if (const int rc = begin_call(lm, st)) return rc; // a _device call may still read the staging planes
    const size_t n = (size_t)lm->width * (size_t)lm->height;
    HIPCHK(hipMemcpyAsync(lm->d_host_rgba, rgba, n * 16u, hipMemcpyHostToDevice, st));
    if (variance) HIPCHK(hipMemcpyAsync(lm->d_host_var_in, variance, n * 4u, hipMemcpyHostToDevice, st));
    if (const int rc = filter_enqueue(lm, f, lm->d_host_rgba, variance ? lm->d_host_var_in : nullptr, lm->d_host_rgba,
                                      out_variance ? lm->d_host_var_out : nullptr, st))
        return rc;
    return host_results(lm, lm->d_host_rgba, out_rgba, out_variance, nullptr);
}

int rt_lightmap_filter_device(rt_lightmap* lm, const rt_lightmap_filter_params* f, const void* d_rgba, const void* d_variance, void* d_out_rgba,
                              void* d_out_variance, void* stream) {
    if (const int rc = filter_check(lm, f, d_rgba, d_variance, d_out_rgba)) return rc;
    if (const int rc = begin_call(lm, (hipStream_t)stream)) return rc;
    return filter_enqueue(lm, f, (const float4*)d_rgba, (const float*)d_variance, (float4*)d_out_rgba, (float*)d_out_variance, (hipStream_t)stream);
}

} // extern "C"
