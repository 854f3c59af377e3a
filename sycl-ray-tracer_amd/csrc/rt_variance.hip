// rt_variance.hip — the variance-guided denoiser (after SVGF: Schied et al., HPG 2017): rt_denoise_variance[_device], rt_denoise_guided[_device]
// and their kernels, for a denoiser created with RT_DENOISER_VARIANCE. The arithmetic is the contract stated at rt_denoise_variance and
// rt_denoise_guided in include/rt_mi355x.h; the numpy models that pin it bit for bit are tests/test_svgf.py: variance_model, guided_model.
//
// The launches have k_atrous's shape (rt_denoise.hip): a workgroup is 64 x 4 pixels, a wave one row of 64 consecutive pixels, one launch per
// iteration, no atomics, no grid synchronisation, no LDS. Between iterations the colour's variance rides in .w of the colour ping-pong planes: a
// tap's bytes are k_atrous's. The first launch takes it from the caller's variance plane (4 bytes more per tap, once). The 3 x 3 prefilter of the
// centre pixel's variance reads its 9 values straight from memory: at step 1 they are among the taps' own addresses, at larger steps they are
// the .w of the wave's own row and the rows beside it.
#include "rt_denoiser.h"

namespace {

constexpr float kLumEps = 1e-8f;
// the prefilter's weights per axis: 1/4, 1/2, 1/4
__constant__ float kPreK[3] = {0.25f, 0.5f, 0.25f};

RT_DEV float luminance(float4 L) { return (L.x * 0.2126f + L.y * 0.7152f) + L.z * 0.0722f; }

// The variance of every pixel's luminance: from the temporal moments where the history is long enough (mom and hist given, hist >= min_hist), else
// over the 7 x 7 window weighted by the guides. kn / kx / ka: the guides' coefficients (0 = that term left out, its guide not read).
__global__ void __launch_bounds__(256) k_variance(const float4* __restrict__ frame, const float4* __restrict__ alb, const float4* __restrict__ nrm,
                                                   const float4* __restrict__ pos, const float2* __restrict__ mom, const float* __restrict__ hist,
                                                   int32_t W, int32_t H, float kn, float kx, float ka, float min_hist, float* __restrict__ out_var) {
    const uint32_t tiles_x = ((uint32_t)W + 63u) / 64u;
    const int32_t x = (int32_t)((blockIdx.x % tiles_x) * 64u + threadIdx.x), y = (int32_t)((blockIdx.x / tiles_x) * 4u + threadIdx.y);
    if (x >= W || y >= H) return;
    const int32_t p = y * W + x;
    if (mom && hist[p] >= min_hist) {
        const float2 m = mom[p];
        out_var[p] = __builtin_fmaxf(m.y - m.x * m.x, 0.0f);
        return;
    }
    const float4 Pp = pos[p];
    const float4 Np = kn != 0.0f ? nrm[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 Ap = ka != 0.0f ? alb[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool hit_p = __builtin_isfinite(Pp.w);
    float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
        const int32_t qy = y + dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int32_t qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const int32_t q = qy * W + qx;
            const float4 Pq = pos[q];
            if (__builtin_isfinite(Pq.w) != hit_p) continue;
            float E = 0.0f;
            if (kn != 0.0f) E = E + dot_diff(Np, nrm[q]) * kn;
            if (kx != 0.0f) E = E + dot_diff(Pp, Pq) * kx;
            if (ka != 0.0f) E = E + dot_diff(Ap, alb[q]) * ka;
            const float w = exp_m(-E);
            const float lq = luminance(squared(frame[q]));
            s1 = s1 + w * lq, s2 = s2 + w * (lq * lq);
            ws = ws + w;
        }
    }
    const float m1 = s1 / ws, m2 = s2 / ws; // ws >= 1: the centre tap's weight
    out_var[p] = __builtin_fmaxf(m2 - m1 * m1, 0.0f);
}

// One variance-guided a-trous iteration with step `step`. use_l: the luminance term is on (sigma_l finite); kn / kx / ka as k_atrous's.
// SQUARE: `in` is the frame (rgb = sqrt(mean)), squared as it is loaded, and the variance is var_in's; otherwise the variance is in.w.
// LAST: writes out (may be null), out_u8 (may be null) and out_var (may be null); otherwise out = (L', var').
template <bool SQUARE, bool LAST>
__global__ void __launch_bounds__(256) k_atrous_guided(const float4* __restrict__ in, const float* __restrict__ var_in, const float4* __restrict__ alb,
                                                        const float4* __restrict__ nrm, const float4* __restrict__ pos, int32_t W, int32_t H,
                                                        int32_t step, int32_t use_l, float sigma_l, float kn, float kx, float ka,
                                                        float4* __restrict__ out, uchar4* __restrict__ out_u8, float* __restrict__ out_var) {
    const uint32_t tiles_x = ((uint32_t)W + 63u) / 64u;
    const int32_t x = (int32_t)((blockIdx.x % tiles_x) * 64u + threadIdx.x), y = (int32_t)((blockIdx.x / tiles_x) * 4u + threadIdx.y);
    if (x >= W || y >= H) return;
    const int32_t p = y * W + x;
    const float4 Lp = SQUARE ? squared(in[p]) : in[p];
    const float4 Pp = pos[p];
    const float4 Np = kn != 0.0f ? nrm[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 Ap = ka != 0.0f ? alb[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool hit_p = __builtin_isfinite(Pp.w);
    const float lp = luminance(Lp);
    float kl = 0.0f;
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
            const float vq = SQUARE ? var_in[q] : Cq.w;
            float E = 0.0f;
            if (use_l) E = E + __builtin_fabsf(lp - luminance(Lq)) * kl;
            if (kn != 0.0f) E = E + dot_diff(Np, nrm[q]) * kn;
            if (kx != 0.0f) E = E + dot_diff(Pp, Pq) * kx;
            if (ka != 0.0f) E = E + dot_diff(Ap, alb[q]) * ka;
            const float w = (kTapH[dy + 2] * kTapH[dx + 2]) * exp_m(-E);
            sx = sx + w * Lq.x, sy = sy + w * Lq.y, sz = sz + w * Lq.z;
            wsum = wsum + w;
            sv = sv + (w * w) * vq;
        }
    }
    const float lx = sx / wsum, ly = sy / wsum, lz = sz / wsum; // wsum >= 9/64 where the centre's E is 0 (see the header for a NaN centre)
    const float var = sv / (wsum * wsum);
    if (!LAST) {
        out[p] = make_float4(lx, ly, lz, var);
        return;
    }
    const float fx = __builtin_sqrtf(lx), fy = __builtin_sqrtf(ly), fz = __builtin_sqrtf(lz);
    if (out) out[p] = make_float4(fx, fy, fz, 1.0f);
    if (out_u8) out_u8[p] = make_uchar4(to_unorm8(fx), to_unorm8(fy), to_unorm8(fz), 255);
    if (out_var) out_var[p] = var;
}

// iterations = 0: the frame as it is (out null where it aliases the frame), its unorm8 image, and the variance as it is
__global__ void __launch_bounds__(256) k_guided_copy(const float4* __restrict__ in, const float* __restrict__ var_in, int32_t n,
                                                      float4* __restrict__ out, uchar4* __restrict__ out_u8, float* __restrict__ out_var) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)n) return;
    const float4 f = in[i];
    if (out) out[i] = f;
    if (out_u8) out_u8[i] = make_uchar4(to_unorm8(f.x), to_unorm8(f.y), to_unorm8(f.z), 255);
    if (out_var) out_var[i] = var_in[i];
}

// (the entry points judge the parameters first: they need no denoiser)
int check_params(const rt_denoise_var_params* p) {
    if (!p) return fail(RT_ERR_INVALID, "null parameters");
    if (p->iterations > kMaxIterations) return fail(RT_ERR_INVALID, "iterations must be 0 .. 10");
    const float s[4] = {p->sigma_luminance, p->sigma_normal, p->sigma_position, p->sigma_albedo};
    for (float v : s)
        if (!(v >= kMinSigma)) return fail(RT_ERR_INVALID, "every sigma must be at least 1e-6 (+inf ignores its guide); NaN is refused");
    return RT_OK;
}

int check_flag(const rt_denoiser* d) {
    if (!(d->flags & RT_DENOISER_VARIANCE)) return fail(RT_ERR_INVALID, "the denoiser was created without RT_DENOISER_VARIANCE (rt_denoiser_create_ex)");
    return RT_OK;
}

dim3 tile_grid(const rt_denoiser* d) { // W * H < 2^31 (rt_denoiser_create): the tile count and every thread index fit in 32 bits
    return dim3((((uint32_t)d->width + 63u) / 64u) * (((uint32_t)d->height + 3u) / 4u));
}

// PRE: the arguments were checked; all pointers are device pointers on d->device (mom and hist both null or both given)
int enqueue_variance(rt_denoiser* d, const rt_denoise_var_params* p, const float4* frame, const float4* alb, const float4* nrm, const float4* pos,
                     const float2* mom, const float* hist, float* out_var, hipStream_t st) {
    HIPCHK(hipSetDevice(d->device));
    if (d->recorded) HIPCHK(hipStreamWaitEvent(st, d->ev_last, 0));
    hipLaunchKernelGGL(k_variance, tile_grid(d), dim3(64, 4), 0, st, frame, alb, nrm, pos, mom, hist, d->width, d->height,
                       coefficient(p->sigma_normal), coefficient(p->sigma_position), coefficient(p->sigma_albedo), (float)p->min_history, out_var);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(d->ev_last, st));
    d->recorded = true;
    return RT_OK;
}

// PRE: as enqueue_variance's
int enqueue_guided(rt_denoiser* d, const rt_denoise_var_params* p, const float4* frame, const float4* alb, const float4* nrm, const float4* pos,
                   const float* var, float4* out_f32, uchar4* out_u8, float* out_var, hipStream_t st) {
    HIPCHK(hipSetDevice(d->device));
    if (d->recorded) HIPCHK(hipStreamWaitEvent(st, d->ev_last, 0)); // the previous call (any stream) is done with the scratch
    const int32_t W = d->width, H = d->height, n = W * H;
    const uint32_t iters = p->iterations;
    if (iters == 0) {
        hipLaunchKernelGGL(k_guided_copy, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, st, frame, var, n, out_f32 == frame ? nullptr : out_f32,
                           out_u8, out_var);
        HIPCHK(hipGetLastError());
    } else {
        const int32_t use_l = std::isinf(p->sigma_luminance) ? 0 : 1;
        const float sl = p->sigma_luminance, kn = coefficient(p->sigma_normal);
        const float kx = coefficient(p->sigma_position), ka = coefficient(p->sigma_albedo);
        const float4* src = frame;
        if (iters == 1 && out_f32 == frame) { // the one launch would read the frame while writing it: it reads a copy
            HIPCHK(hipMemcpyAsync(d->d_scratch[1], frame, (size_t)n * 16u, hipMemcpyDeviceToDevice, st));
            src = d->d_scratch[1];
        }
        const dim3 grid = tile_grid(d), block(64, 4);
        for (uint32_t i = 0; i < iters; ++i) {
            const bool first = i == 0, last = i + 1 == iters;
            float4* dst = last ? out_f32 : d->d_scratch[i & 1u];
            uchar4* u8 = last ? out_u8 : nullptr;
            float* ov = last ? out_var : nullptr;
            const float kni = std::ldexp(kn, -2 * (int)i); // the normal term is divided by the step squared, as rt_denoise's
            const int32_t step = 1 << i;
            if (first && last) hipLaunchKernelGGL((k_atrous_guided<true, true>), grid, block, 0, st, src, var, alb, nrm, pos, W, H, step, use_l, sl, kni, kx, ka, dst, u8, ov);
            else if (first) hipLaunchKernelGGL((k_atrous_guided<true, false>), grid, block, 0, st, src, var, alb, nrm, pos, W, H, step, use_l, sl, kni, kx, ka, dst, u8, ov);
            else if (last) hipLaunchKernelGGL((k_atrous_guided<false, true>), grid, block, 0, st, src, var, alb, nrm, pos, W, H, step, use_l, sl, kni, kx, ka, dst, u8, ov);
            else hipLaunchKernelGGL((k_atrous_guided<false, false>), grid, block, 0, st, src, var, alb, nrm, pos, W, H, step, use_l, sl, kni, kx, ka, dst, u8, ov);
            HIPCHK(hipGetLastError());
            src = dst;
        }
    }
    HIPCHK(hipEventRecord(d->ev_last, st));
    d->recorded = true;
    return RT_OK;
}

// the four input planes of a host call -> the staging planes
int stage_inputs(rt_denoiser* d, const float* rgba_f32, const float* albedo, const float* normal, const float* position, hipStream_t st) {
    const size_t n = (size_t)d->width * (size_t)d->height, bytes = n * 16u;
    float4* in = d->d_host_in;
    if (d->recorded) HIPCHK(hipStreamWaitEvent(st, d->ev_last, 0)); // a _device call may still read the staging planes' neighbours
    HIPCHK(hipMemcpyAsync(in, rgba_f32, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + n, albedo, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + 2 * n, normal, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + 3 * n, position, bytes, hipMemcpyHostToDevice, st));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_denoise_variance(rt_denoiser* d, const rt_denoise_var_params* p, const float* rgba_f32, const float* albedo, const float* normal,
                        const float* position, const float* moments, const float* history_len, float* out_variance) {
    if (const int rc = check_params(p)) return rc;
    if (!d || !rgba_f32 || !albedo || !normal || !position || !out_variance) return fail(RT_ERR_INVALID, "null argument");
    if ((moments == nullptr) != (history_len == nullptr)) return fail(RT_ERR_INVALID, "moments and history_len go together: both or neither");
    if (const int rc = check_flag(d)) return rc;
    HIPCHK(hipSetDevice(d->device));
    const size_t n = (size_t)d->width * (size_t)d->height;
    float4* in = d->d_host_in;
    hipStream_t st = d->stream;
    if (const int rc = stage_inputs(d, rgba_f32, albedo, normal, position, st)) return rc;
    if (moments) {
        HIPCHK(hipMemcpyAsync(d->d_host_mom, moments, n * 8u, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d->d_host_len, history_len, n * 4u, hipMemcpyHostToDevice, st));
    }
    if (const int rc = enqueue_variance(d, p, in, in + n, in + 2 * n, in + 3 * n, moments ? d->d_host_mom : nullptr,
                                        moments ? d->d_host_len : nullptr, d->d_host_var_out, st))
        return rc;
    HIPCHK(hipMemcpyAsync(out_variance, d->d_host_var_out, n * 4u, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_denoise_variance_device(rt_denoiser* d, const rt_denoise_var_params* p, const void* d_rgba_f32, const void* d_albedo, const void* d_normal,
                               const void* d_position, const void* d_moments, const void* d_history_len, void* d_out_variance, void* stream) {
    if (const int rc = check_params(p)) return rc;
    if (!d || !d_rgba_f32 || !d_albedo || !d_normal || !d_position || !d_out_variance) return fail(RT_ERR_INVALID, "null argument");
    if ((d_moments == nullptr) != (d_history_len == nullptr)) return fail(RT_ERR_INVALID, "moments and history_len go together: both or neither");
    if (const int rc = check_flag(d)) return rc;
    return enqueue_variance(d, p, (const float4*)d_rgba_f32, (const float4*)d_albedo, (const float4*)d_normal, (const float4*)d_position,
                            (const float2*)d_moments, (const float*)d_history_len, (float*)d_out_variance, (hipStream_t)stream);
}

int rt_denoise_guided(rt_denoiser* d, const rt_denoise_var_params* p, const float* rgba_f32, const float* albedo, const float* normal,
                      const float* position, const float* variance, float* out_f32, uint8_t* out_u8, float* out_variance) {
    if (const int rc = check_params(p)) return rc;
    if (!out_f32 && !out_u8) return fail(RT_ERR_INVALID, "out_f32 and out_u8 are both null");
    if (!d || !rgba_f32 || !albedo || !normal || !position || !variance) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = check_flag(d)) return rc;
    HIPCHK(hipSetDevice(d->device));
    const size_t n = (size_t)d->width * (size_t)d->height, bytes = n * 16u;
    float4* in = d->d_host_in;
    hipStream_t st = d->stream;
    if (const int rc = stage_inputs(d, rgba_f32, albedo, normal, position, st)) return rc;
    HIPCHK(hipMemcpyAsync(d->d_host_var_in, variance, n * 4u, hipMemcpyHostToDevice, st));
    if (const int rc = enqueue_guided(d, p, in, in + n, in + 2 * n, in + 3 * n, d->d_host_var_in, out_f32 ? d->d_host_f32 : nullptr,
                                      out_u8 ? (uchar4*)d->d_host_u8 : nullptr, out_variance ? d->d_host_var_out : nullptr, st))
        return rc;
    if (out_f32) HIPCHK(hipMemcpyAsync(out_f32, d->d_host_f32, bytes, hipMemcpyDeviceToHost, st));
    if (out_u8) HIPCHK(hipMemcpyAsync(out_u8, d->d_host_u8, n * 4u, hipMemcpyDeviceToHost, st));
    if (out_variance) HIPCHK(hipMemcpyAsync(out_variance, d->d_host_var_out, n * 4u, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_denoise_guided_device(rt_denoiser* d, const rt_denoise_var_params* p, const void* d_rgba_f32, const void* d_albedo, const void* d_normal,
                             const void* d_position, const void* d_variance, void* d_out_f32, void* d_out_u8, void* d_out_variance, void* stream) {
    if (const int rc = check_params(p)) return rc;
    if (!d_out_f32 && !d_out_u8) return fail(RT_ERR_INVALID, "out_f32 and out_u8 are both null");
    if (!d || !d_rgba_f32 || !d_albedo || !d_normal || !d_position || !d_variance) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = check_flag(d)) return rc;
    return enqueue_guided(d, p, (const float4*)d_rgba_f32, (const float4*)d_albedo, (const float4*)d_normal, (const float4*)d_position,
                          (const float*)d_variance, (float4*)d_out_f32, (uchar4*)d_out_u8, (float*)d_out_variance, (hipStream_t)stream);
}

} // extern "C"
