// rt_denoise.hip — the edge-avoiding a-trous denoiser (Dammertz, Sewtz, Hanika, Lensch, HPG 2010): rt_denoiser_create[_ex] / _destroy,
// rt_denoise[_device] and their kernels. The filter's arithmetic is the contract stated at rt_denoise in include/rt_mi355x.h; the
// numpy model that pins it bit for bit is tests/test_denoise.py: denoise_model.
//
// One launch per iteration (the kernel boundary is the only hand-off: a tap of iteration i + 1 reads what other workgroups wrote in
// iteration i). The first launch squares the frame as it loads it (linear radiance), the last writes sqrt and the unorm8 image; between
// them linear colour ping-pongs through the denoiser's two float4 scratch planes. A workgroup is 64 x 4 pixels, a wave one row of 64
// consecutive pixels: every tap's 16-byte loads of colour and guides are one contiguous 1 KB row segment per wave.
#include "rt_denoiser.h"

namespace {

// one a-trous iteration with step `step`; kc / kn / kx / ka: this iteration's coefficients (0 = that term left out, its guide not read)
// SQUARE: `in` is the frame (rgb = sqrt(mean)), squared as it is loaded; LAST: writes out_f32 (may be null) and out_u8 (may be null)
template <bool SQUARE, bool LAST>
__global__ void __launch_bounds__(256) k_atrous(const float4* __restrict__ in, const float4* __restrict__ alb, const float4* __restrict__ nrm,
                                                 const float4* __restrict__ pos, int32_t W, int32_t H, int32_t step, float kc, float kn, float kx,
                                                 float ka, float4* __restrict__ out, uchar4* __restrict__ out_u8) {
    // a 1-D grid of 64 x 4 tiles, row-major (a second grid dimension would bound the image's height)
    const uint32_t tiles_x = ((uint32_t)W + 63u) / 64u;
    const int32_t x = (int32_t)((blockIdx.x % tiles_x) * 64u + threadIdx.x), y = (int32_t)((blockIdx.x / tiles_x) * 4u + threadIdx.y);
    if (x >= W || y >= H) return;
    const int32_t p = y * W + x;
    const float4 Lp = SQUARE ? squared(in[p]) : in[p];
    const float4 Pp = pos[p];
    const float4 Np = kn != 0.0f ? nrm[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 Ap = ka != 0.0f ? alb[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool hit_p = __builtin_isfinite(Pp.w);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
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
            const float4 Lq = SQUARE ? squared(in[q]) : in[q];
            float E = 0.0f;
            if (kc != 0.0f) E = E + dot_diff(Lp, Lq) * kc;
            if (kn != 0.0f) E = E + dot_diff(Np, nrm[q]) * kn;
            if (kx != 0.0f) E = E + dot_diff(Pp, Pq) * kx;
            if (ka != 0.0f) E = E + dot_diff(Ap, alb[q]) * ka;
            const float w = (kTapH[dy + 2] * kTapH[dx + 2]) * exp_m(-E);
            sx = sx + w * Lq.x, sy = sy + w * Lq.y, sz = sz + w * Lq.z;
            wsum = wsum + w;
        }
    }
    const float lx = sx / wsum, ly = sy / wsum, lz = sz / wsum; // wsum >= 9/64: the centre tap's weight
    if (!LAST) {
        out[p] = make_float4(lx, ly, lz, 1.0f);
        return;
    }
    const float fx = __builtin_sqrtf(lx), fy = __builtin_sqrtf(ly), fz = __builtin_sqrtf(lz);
    if (out) out[p] = make_float4(fx, fy, fz, 1.0f);
    if (out_u8) out_u8[p] = make_uchar4(to_unorm8(fx), to_unorm8(fy), to_unorm8(fz), 255);
}

// iterations = 0: the frame as it is (out null where it aliases the frame) and its unorm8 image
__global__ void __launch_bounds__(256) k_denoise_copy(const float4* __restrict__ in, int32_t n, float4* __restrict__ out, uchar4* __restrict__ out_u8) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)n) return;
    const float4 f = in[i];
    if (out) out[i] = f;
    if (out_u8) out_u8[i] = make_uchar4(to_unorm8(f.x), to_unorm8(f.y), to_unorm8(f.z), 255);
}

int check_params(const rt_denoise_params* p) {
    if (!p) return fail(RT_ERR_INVALID, "null parameters");
    if (p->iterations > kMaxIterations) return fail(RT_ERR_INVALID, "iterations must be 0 .. 10");
    const float s[4] = {p->sigma_color, p->sigma_normal, p->sigma_position, p->sigma_albedo};
    for (float v : s)
        if (!(v >= kMinSigma)) return fail(RT_ERR_INVALID, "every sigma must be at least 1e-6 (+inf ignores its guide); NaN is refused");
    return RT_OK;
}

// PRE: the arguments were checked; all pointers are device pointers on d->device
int enqueue(rt_denoiser* d, const rt_denoise_params* p, const float4* frame, const float4* alb, const float4* nrm, const float4* pos,
            float4* out_f32, uchar4* out_u8, hipStream_t st) {
    HIPCHK(hipSetDevice(d->device));
    if (d->recorded) HIPCHK(hipStreamWaitEvent(st, d->ev_last, 0)); // the previous call (any stream) is done with the scratch
    const int32_t W = d->width, H = d->height, n = W * H;
    const uint32_t iters = p->iterations;
    if (iters == 0) {
        hipLaunchKernelGGL(k_denoise_copy, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, st, frame, n,
                           out_f32 == frame ? nullptr : out_f32, out_u8);
        HIPCHK(hipGetLastError());
    } else {
        const float kc = coefficient(p->sigma_color), kn = coefficient(p->sigma_normal);
        const float kx = coefficient(p->sigma_position), ka = coefficient(p->sigma_albedo);
        const float4* src = frame;
        if (iters == 1 && out_f32 == frame) { // the one launch would read the frame while writing it: it reads a copy
            HIPCHK(hipMemcpyAsync(d->d_scratch[1], frame, (size_t)n * 16u, hipMemcpyDeviceToDevice, st));
            src = d->d_scratch[1];
        }
        // W * H < 2^31 (rt_denoiser_create): the tile count and every thread index fit in 32 bits
        const dim3 grid((((uint32_t)W + 63u) / 64u) * (((uint32_t)H + 3u) / 4u)), block(64, 4);
        for (uint32_t i = 0; i < iters; ++i) {
            const bool first = i == 0, last = i + 1 == iters;
            float4* dst = last ? out_f32 : d->d_scratch[i & 1u];
            uchar4* u8 = last ? out_u8 : nullptr;
            // the colour sigma halves per iteration (its coefficient x 4), the normal term is divided by the step squared
            const float kci = std::ldexp(kc, 2 * (int)i), kni = std::ldexp(kn, -2 * (int)i);
            const int32_t step = 1 << i;
            if (first && last) hipLaunchKernelGGL((k_atrous<true, true>), grid, block, 0, st, src, alb, nrm, pos, W, H, step, kci, kni, kx, ka, dst, u8);
            else if (first) hipLaunchKernelGGL((k_atrous<true, false>), grid, block, 0, st, src, alb, nrm, pos, W, H, step, kci, kni, kx, ka, dst, u8);
            else if (last) hipLaunchKernelGGL((k_atrous<false, true>), grid, block, 0, st, src, alb, nrm, pos, W, H, step, kci, kni, kx, ka, dst, u8);
            else hipLaunchKernelGGL((k_atrous<false, false>), grid, block, 0, st, src, alb, nrm, pos, W, H, step, kci, kni, kx, ka, dst, u8);
            HIPCHK(hipGetLastError());
            src = dst;
        }
    }
    HIPCHK(hipEventRecord(d->ev_last, st));
    d->recorded = true;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_denoiser_create(int device, int32_t width, int32_t height, rt_denoiser** out) {
    return rt_denoiser_create_ex(device, width, height, 0u, out);
}

int rt_denoiser_create_ex(int device, int32_t width, int32_t height, uint32_t flags, rt_denoiser** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (device < 0) return fail(RT_ERR_INVALID, "device index out of range");
    if (flags & ~RT_DENOISER_VARIANCE) return fail(RT_ERR_INVALID, "unknown denoiser flag");
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "width and height must be positive");
    if ((uint64_t)width * (uint64_t)height > 0x7fffffffull) return fail(RT_ERR_INVALID, "image too large (W x H must stay below 2^31)");
    // k_atrous's 1-D grid of 64 x 4 tiles: its threads, padding included, must stay below 2^32 (only very narrow images reach that)
    if (((uint64_t)width + 63u) / 64u * (((uint64_t)height + 3u) / 4u) * 256u > 0xffffffffull)
        return fail(RT_ERR_INVALID, "image shape too narrow and tall for the filter's launch grid");
    const int rc = device_ok(device);
    if (rc != RT_OK) return rc;
    return no_throw([&]() -> int {
        rt_denoiser* d = new rt_denoiser;
        d->device = device, d->width = width, d->height = height, d->flags = flags;
        const size_t n = (size_t)width * (size_t)height, bytes = n * 16u;
        if (hipMalloc((void**)&d->d_scratch[0], bytes) != hipSuccess || hipMalloc((void**)&d->d_scratch[1], bytes) != hipSuccess ||
            hipMalloc((void**)&d->d_host_in, 4 * bytes) != hipSuccess || hipMalloc((void**)&d->d_host_f32, bytes) != hipSuccess ||
            hipMalloc((void**)&d->d_host_u8, n * 4u) != hipSuccess ||
            ((flags & RT_DENOISER_VARIANCE) &&
             (hipMalloc((void**)&d->d_host_var_in, n * 4u) != hipSuccess || hipMalloc((void**)&d->d_host_var_out, n * 4u) != hipSuccess ||
              hipMalloc((void**)&d->d_host_mom, n * 8u) != hipSuccess || hipMalloc((void**)&d->d_host_len, n * 4u) != hipSuccess))) {
            rt_denoiser_destroy(d);
            return fail(RT_ERR_OOM, "hipMalloc of the denoiser's scratch and staging failed");
        }
        if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&d->ev_last, hipEventDisableTiming) != hipSuccess) {
            rt_denoiser_destroy(d);
            return fail(RT_ERR_HIP, "hipStreamCreate / hipEventCreate failed");
        }
        *out = d;
        return (int)RT_OK;
    });
}

void rt_denoiser_destroy(rt_denoiser* d) {
    if (!d) return;
    if (d->device >= 0 && hipSetDevice(d->device) == hipSuccess) {
        if (d->recorded) (void)hipEventSynchronize(d->ev_last);
        (void)hipFree(d->d_scratch[0]), (void)hipFree(d->d_scratch[1]);
        (void)hipFree(d->d_host_in), (void)hipFree(d->d_host_f32), (void)hipFree(d->d_host_u8);
        (void)hipFree(d->d_host_var_in), (void)hipFree(d->d_host_var_out), (void)hipFree(d->d_host_mom), (void)hipFree(d->d_host_len);
        if (d->ev_last) (void)hipEventDestroy(d->ev_last);
        if (d->stream) (void)hipStreamDestroy(d->stream);
    }
    delete d;
}

int rt_denoise(rt_denoiser* d, const rt_denoise_params* p, const float* rgba_f32, const float* albedo, const float* normal, const float* position,
               float* out_f32, uint8_t* out_u8) {
    if (!d || !rgba_f32 || !albedo || !normal || !position) return fail(RT_ERR_INVALID, "null argument");
    if (!out_f32 && !out_u8) return fail(RT_ERR_INVALID, "out_f32 and out_u8 are both null");
    if (const int rc = check_params(p)) return rc;
    HIPCHK(hipSetDevice(d->device));
    const size_t n = (size_t)d->width * (size_t)d->height, bytes = n * 16u;
    float4* in = d->d_host_in;
    hipStream_t st = d->stream;
    if (d->recorded) HIPCHK(hipStreamWaitEvent(st, d->ev_last, 0)); // a _device call may still read the staging planes' neighbours
    HIPCHK(hipMemcpyAsync(in, rgba_f32, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + n, albedo, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + 2 * n, normal, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + 3 * n, position, bytes, hipMemcpyHostToDevice, st));
    if (const int rc = enqueue(d, p, in, in + n, in + 2 * n, in + 3 * n, out_f32 ? d->d_host_f32 : nullptr,
                               out_u8 ? (uchar4*)d->d_host_u8 : nullptr, st))
        return rc;
    if (out_f32) HIPCHK(hipMemcpyAsync(out_f32, d->d_host_f32, bytes, hipMemcpyDeviceToHost, st));
    if (out_u8) HIPCHK(hipMemcpyAsync(out_u8, d->d_host_u8, n * 4u, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_denoise_device(rt_denoiser* d, const rt_denoise_params* p, const void* d_rgba_f32, const void* d_albedo, const void* d_normal,
                      const void* d_position, void* d_out_f32, void* d_out_u8, void* stream) {
    if (!d || !d_rgba_f32 || !d_albedo || !d_normal || !d_position) return fail(RT_ERR_INVALID, "null argument");
    if (!d_out_f32 && !d_out_u8) return fail(RT_ERR_INVALID, "out_f32 and out_u8 are both null");
    if (const int rc = check_params(p)) return rc;
    return enqueue(d, p, (const float4*)d_rgba_f32, (const float4*)d_albedo, (const float4*)d_normal, (const float4*)d_position,
                   (float4*)d_out_f32, (uchar4*)d_out_u8, (hipStream_t)stream);
}

} // extern "C"
