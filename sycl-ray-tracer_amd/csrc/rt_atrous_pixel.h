// rt_atrous_pixel.h — what one thread of an a-trous iteration does, for k_atrous (rt_denoise.hip: one global colour sigma) and k_atrous_guided
// (rt_variance.hip: the luminance term scaled by the pixel's prefiltered variance, and the variance filtered along), and the host loop that
// runs the iterations of either. The two kernels stay in their units under their names: each is a one-line call of atrous_pixel, and its
// listing is the one it had as a text of its own (EXPERIMENTS.md, "One a-trous pixel text").
#pragma once
#include <type_traits>

#include "rt_denoiser.h"

namespace {

constexpr float kLumEps = 1e-8f;
// the variance prefilter's weights per axis: 1/4, 1/2, 1/4
__constant__ float kPreK[3] = {0.25f, 0.5f, 0.25f};

RT_DEV float luminance(float4 L) { return (L.x * 0.2126f + L.y * 0.7152f) + L.z * 0.0722f; }

// One a-trous iteration with step `step`, at the thread's pixel. kn / kx / ka: this iteration's guide coefficients (0 = that term left out, its
// guide not read).
// SQUARE: `in` is the frame (rgb = sqrt(mean)), squared as it is loaded; LAST: writes sqrt to out (may be null) and out_u8 (may be null).
// GUIDED = false (rt_denoise): kc is the colour term's coefficient (0 = left out); out.w = 1. var_in, use_l, sigma_l, out_var are not read.
// GUIDED = true (rt_denoise_guided): use_l: the luminance term is on (sigma_l finite), scaled by the 3 x 3 prefilter of the variance at p; the
// variance is var_in's with SQUARE, else in.w; it leaves in out.w, or with LAST in out_var (may be null). kc is not read.
template <bool GUIDED, bool SQUARE, bool LAST>
RT_DEV void atrous_pixel(const float4* __restrict__ in, const float* __restrict__ var_in, const float4* __restrict__ alb,
                         const float4* __restrict__ nrm, const float4* __restrict__ pos, int32_t W, int32_t H, int32_t step, int32_t use_l,
                         float sigma_l, float kc, float kn, float kx, float ka, float4* __restrict__ out, uchar4* __restrict__ out_u8,
                         float* __restrict__ out_var) {
    int32_t x, y;
    if (!tile_pixel(W, H, &x, &y)) return;
    const int32_t p = y * W + x;
    const float4 Lp = SQUARE ? squared(in[p]) : in[p];
    const float4 Pp = pos[p];
    const float4 Np = kn != 0.0f ? nrm[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 Ap = ka != 0.0f ? alb[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool hit_p = __builtin_isfinite(Pp.w);
    float lp = 0.0f, kl = 0.0f;
    if constexpr (GUIDED) {
        lp = luminance(Lp);
        if (use_l) { // the 3 x 3 prefilter of the variance at p, addresses clamped into the image
            float g = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int32_t qy = min(max(y + dy, 0), H - 1);
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int32_t q = qy * W + min(max(x + dx, 0), W - 1);
                    const float v = SQUARE ? var_in[q] : in[q].w;
                    g = g + (kPreK[dy + 1] * kPreK[dx + 1]) * v;
                }
            }
            kl = 1.0f / (sigma_l * __builtin_sqrtf(g) + kLumEps);
        }
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
            const float4 Pq = pos[q];
            if (__builtin_isfinite(Pq.w) != hit_p) continue;
            const float4 Cq = in[q];
            const float4 Lq = SQUARE ? squared(Cq) : Cq;
            float vq = 0.0f; // (loaded here, right behind the colour: placed behind the weight, the SQUARE kernels grow by 200 bytes)
            if constexpr (GUIDED) vq = SQUARE ? var_in[q] : Cq.w;
            float E = 0.0f;
            if constexpr (GUIDED) {
                if (use_l) E = E + __builtin_fabsf(lp - luminance(Lq)) * kl;
            } else {
                if (kc != 0.0f) E = E + dot_diff(Lp, Lq) * kc;
            }
            if (kn != 0.0f) E = E + dot_diff(Np, nrm[q]) * kn;
            if (kx != 0.0f) E = E + dot_diff(Pp, Pq) * kx;
            if (ka != 0.0f) E = E + dot_diff(Ap, alb[q]) * ka;
            const float w = (kTapH[dy + 2] * kTapH[dx + 2]) * exp_m(-E);
            sx = sx + w * Lq.x, sy = sy + w * Lq.y, sz = sz + w * Lq.z;
            wsum = wsum + w;
            if constexpr (GUIDED) sv = sv + (w * w) * vq;
        }
    }
    // wsum >= 9/64 where the centre tap's E is 0: always without the luminance term (see include/rt_mi355x.h for a NaN centre with it)
    const float lx = sx / wsum, ly = sy / wsum, lz = sz / wsum;
    const float var = GUIDED ? sv / (wsum * wsum) : 1.0f;
    if (!LAST) {
        out[p] = make_float4(lx, ly, lz, var);
        return;
    }
    const float fx = __builtin_sqrtf(lx), fy = __builtin_sqrtf(ly), fz = __builtin_sqrtf(lz);
    if (out) out[p] = make_float4(fx, fy, fz, 1.0f);
    if (out_u8) out_u8[p] = make_uchar4(to_unorm8(fx), to_unorm8(fy), to_unorm8(fz), 255);
    if constexpr (GUIDED) {
        if (out_var) out_var[p] = var;
    }
}

// The iterations of one filter call (iters >= 1; PRE: the call's bracket is open on st): one launch per iteration, the kernel boundary the only
// hand-off. The first launch reads the frame, the last writes out_f32; between them linear colour ping-pongs through the denoiser's two scratch
// planes. launch(square, last, src, dst, i, kni) enqueues iteration i with step 1 << i on st: square and last are std::bool_constant, the
// kernel's SQUARE and LAST; kni is kn divided by the step squared.
template <typename Launch>
int atrous_iterations(rt_denoiser* d, uint32_t iters, const float4* frame, float4* out_f32, float kn, hipStream_t st, Launch launch) {
    const float4* src = frame;
    if (iters == 1 && out_f32 == frame) { // the one launch would read the frame while writing it: it reads a copy
        HIPCHK(hipMemcpyAsync(d->d_scratch[1], frame, d->pixels() * 16u, hipMemcpyDeviceToDevice, st));
        src = d->d_scratch[1];
    }
    for (uint32_t i = 0; i < iters; ++i) {
        const bool first = i == 0, last = i + 1 == iters;
        float4* dst = last ? out_f32 : d->d_scratch[i & 1u];
        const float kni = std::ldexp(kn, -2 * (int)i);
        if (first && last) launch(std::true_type{}, std::true_type{}, src, dst, i, kni);
        else if (first) launch(std::true_type{}, std::false_type{}, src, dst, i, kni);
        else if (last) launch(std::false_type{}, std::true_type{}, src, dst, i, kni);
        else launch(std::false_type{}, std::false_type{}, src, dst, i, kni);
        HIPCHK(hipGetLastError());
        src = dst;
    }
    return RT_OK;
}

} // namespace
