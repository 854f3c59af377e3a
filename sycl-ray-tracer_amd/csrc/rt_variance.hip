// rt_variance.hip — the variance-guided denoiser (after SVGF: Schied et al., HPG 2017): rt_denoise_variance[_device], rt_denoise_guided[_device]
// and their kernels, for a denoiser created with RT_DENOISER_VARIANCE. The arithmetic is the contract stated at rt_denoise_variance and
// rt_denoise_guided in include/rt_mi355x.h; the numpy models that pin it bit for bit are tests/test_svgf.py: variance_model, guided_model.
//
// The launches have k_atrous's shape (rt_denoise.hip): a workgroup is 64 x 4 pixels, a wave one row of 64 consecutive pixels, one launch per
// iteration, no atomics, no grid synchronisation, no LDS. Between iterations the colour's variance rides in .w of the colour ping-pong planes: a
// tap's bytes are k_atrous's. The first launch takes it from the caller's variance plane (4 bytes more per tap, once). The 3 x 3 prefilter of the
// centre pixel's variance reads its 9 values straight from memory: at step 1 they are among the taps' own addresses, at larger steps they are
// the .w of the wave's own row and the rows beside it. The filter's pixel and the loop over its iterations are rt_atrous_pixel.h's,
// shared with rt_denoise.hip; k_variance's window is its own text.
#include "rt_atrous_pixel.h"

namespace {

// The variance of every pixel's luminance: from the temporal moments where the history is long enough (mom and hist given, hist >= min_hist), else
// over the 7 x 7 window weighted by the guides. kn / kx / ka: the guides' coefficients (0 = that term left out, its guide not read).
__global__ void __launch_bounds__(256) k_variance(const float4* __restrict__ frame, const float4* __restrict__ alb, const float4* __restrict__ nrm,
                                                   const float4* __restrict__ pos, const float2* __restrict__ mom, const float* __restrict__ hist,
                                                   int32_t W, int32_t H, float kn, float kx, float ka, float min_hist, float* __restrict__ out_var) {
    int32_t x, y;
    if (!tile_pixel(W, H, &x, &y)) return;
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

// one variance-guided a-trous iteration with step `step` (rt_atrous_pixel.h); use_l: the luminance term is on (sigma_l finite)
template <bool SQUARE, bool LAST>
__global__ void __launch_bounds__(256) k_atrous_guided(const float4* __restrict__ in, const float* __restrict__ var_in, const float4* __restrict__ alb,
                                                        const float4* __restrict__ nrm, const float4* __restrict__ pos, int32_t W, int32_t H,
                                                        int32_t step, int32_t use_l, float sigma_l, float kn, float kx, float ka,
                                                        float4* __restrict__ out, uchar4* __restrict__ out_u8, float* __restrict__ out_var) {
    atrous_pixel<true, SQUARE, LAST>(in, var_in, alb, nrm, pos, W, H, step, use_l, sigma_l, 0.0f, kn, kx, ka, out, out_u8, out_var);
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

// PRE: the arguments were checked; all pointers are device pointers on d->device (mom and hist both null or both given)
int enqueue_variance(rt_denoiser* d, const rt_denoise_var_params* p, const float4* frame, const float4* alb, const float4* nrm, const float4* pos,
                     const float2* mom, const float* hist, float* out_var, hipStream_t st) {
    if (const int rc = begin_call(d, st)) return rc;
    hipLaunchKernelGGL(k_variance, tile_grid(d->width, d->height), tile_block(), 0, st, frame, alb, nrm, pos, mom, hist, d->width, d->height,
                       coefficient(p->sigma_normal), coefficient(p->sigma_position), coefficient(p->sigma_albedo), (float)p->min_history, out_var);
    return end_call(d, st);
}

// PRE: as enqueue_variance's
int enqueue_guided(rt_denoiser* d, const rt_denoise_var_params* p, const float4* frame, const float4* alb, const float4* nrm, const float4* pos,
                   const float* var, float4* out_f32, uchar4* out_u8, float* out_var, hipStream_t st) {
    if (const int rc = begin_call(d, st)) return rc; // the previous call (any stream) is done with the scratch
    const int32_t W = d->width, H = d->height, n = W * H;
    if (p->iterations == 0) {
        hipLaunchKernelGGL(k_guided_copy, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, st, frame, var, n, out_f32 == frame ? nullptr : out_f32,
                           out_u8, out_var);
    } else {
        const int32_t use_l = std::isinf(p->sigma_luminance) ? 0 : 1;
        const float sl = p->sigma_luminance, kx = coefficient(p->sigma_position), ka = coefficient(p->sigma_albedo);
        const int rc = atrous_iterations(d, p->iterations, frame, out_f32, coefficient(p->sigma_normal), st,
                                         [&](auto square, auto last, const float4* src, float4* dst, uint32_t i, float kni) {
            constexpr bool SQUARE = decltype(square)::value, LAST = decltype(last)::value;
            hipLaunchKernelGGL((k_atrous_guided<SQUARE, LAST>), tile_grid(W, H), tile_block(), 0, st, src, var, alb, nrm, pos, W, H, 1 << i, use_l, sl, kni,
                               kx, ka, dst, LAST ? out_u8 : nullptr, LAST ? out_var : nullptr);
        });
        if (rc != RT_OK) return rc;
    }
    return end_call(d, st);
}

} // namespace

extern "C" {

int rt_denoise_variance(rt_denoiser* d, const rt_denoise_var_params* p, const float* rgba_f32, const float* albedo, const float* normal,
                        const float* position, const float* moments, const float* history_len, float* out_variance) {
    if (const int rc = check_params(p)) return rc;
    if (!d || !rgba_f32 || !albedo || !normal || !position || !out_variance) return fail(RT_ERR_INVALID, "null argument");
    if ((moments == nullptr) != (history_len == nullptr)) return fail(RT_ERR_INVALID, "moments and history_len go together: both or neither");
    if (const int rc = check_flag(d)) return rc;
    hipStream_t st = d->stream;
    if (const int rc = stage_in(d, st, {rgba_f32, albedo, normal, position})) return rc;
    const size_t n = d->pixels();
    const float4* in = d->d_host_in;
    if (moments) {
        HIPCHK(hipMemcpyAsync(d->d_host_mom, moments, n * 8u, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d->d_host_len, history_len, n * 4u, hipMemcpyHostToDevice, st));
    }
    if (const int rc = enqueue_variance(d, p, in, in + n, in + 2 * n, in + 3 * n, moments ? d->d_host_mom : nullptr,
                                        moments ? d->d_host_len : nullptr, d->d_host_var_out, st))
        return rc;
    HIPCHK(hipMemcpyAsync(out_variance, d->d_host_var_out, n * 4u, hipMemcpyDeviceToHost, st));
    return stage_out(d, st, nullptr, nullptr);
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
    hipStream_t st = d->stream;
    if (const int rc = stage_in(d, st, {rgba_f32, albedo, normal, position})) return rc;
    const size_t n = d->pixels();
    const float4* in = d->d_host_in;
    HIPCHK(hipMemcpyAsync(d->d_host_var_in, variance, n * 4u, hipMemcpyHostToDevice, st));
    if (const int rc = enqueue_guided(d, p, in, in + n, in + 2 * n, in + 3 * n, d->d_host_var_in, out_f32 ? d->d_host_f32 : nullptr,
                                      out_u8 ? (uchar4*)d->d_host_u8 : nullptr, out_variance ? d->d_host_var_out : nullptr, st))
        return rc;
    if (out_variance) HIPCHK(hipMemcpyAsync(out_variance, d->d_host_var_out, n * 4u, hipMemcpyDeviceToHost, st));
    return stage_out(d, st, out_f32, out_u8);
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
