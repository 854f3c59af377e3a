// rt_denoise.hip — the edge-avoiding a-trous denoiser (Dammertz, Sewtz, Hanika, Lensch, HPG 2010): rt_denoiser_create[_ex] / _destroy,
// rt_denoise[_device] and their kernels. The filter's arithmetic is the contract stated at rt_denoise in include/rt_mi355x.h; the
// numpy model that pins it bit for bit is tests/test_denoise.py: denoise_model.
//
// One launch per iteration (the kernel boundary is the only hand-off: a tap of iteration i + 1 reads what other workgroups wrote in
// iteration i). The first launch squares the frame as it loads it (linear radiance), the last writes sqrt and the unorm8 image; between
// them linear colour ping-pongs through the denoiser's two float4 scratch planes. A workgroup is 64 x 4 pixels, a wave one row of 64
// consecutive pixels: every tap's 16-byte loads of colour and guides are one contiguous 1 KB row segment per wave.
// What a thread does and the loop over the iterations are rt_atrous_pixel.h's, shared with rt_variance.hip; creation, the bracket of a call
// and the host staging are rt_image_op.h's, shared with the temporal accumulator as well.
#include "rt_atrous_pixel.h"

namespace {

// one a-trous iteration with step `step` (rt_atrous_pixel.h); kc / kn / kx / ka: this iteration's coefficients
template <bool SQUARE, bool LAST>
__global__ void __launch_bounds__(256) k_atrous(const float4* __restrict__ in, const float4* __restrict__ alb, const float4* __restrict__ nrm,
                                                 const float4* __restrict__ pos, int32_t W, int32_t H, int32_t step, float kc, float kn, float kx,
                                                 float ka, float4* __restrict__ out, uchar4* __restrict__ out_u8) {
    atrous_pixel<false, SQUARE, LAST>(in, nullptr, alb, nrm, pos, W, H, step, 0, 0.0f, kc, kn, kx, ka, out, out_u8, nullptr);
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
    if (const int rc = begin_call(d, st)) return rc; // the previous call (any stream) is done with the scratch
    const int32_t W = d->width, H = d->height, n = W * H;
    if (p->iterations == 0) {
        hipLaunchKernelGGL(k_denoise_copy, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, st, frame, n,
                           out_f32 == frame ? nullptr : out_f32, out_u8);
    } else {
        const float kc = coefficient(p->sigma_color), kx = coefficient(p->sigma_position), ka = coefficient(p->sigma_albedo);
        const int rc = atrous_iterations(d, p->iterations, frame, out_f32, coefficient(p->sigma_normal), st,
                                         [&](auto square, auto last, const float4* src, float4* dst, uint32_t i, float kni) {
            constexpr bool SQUARE = decltype(square)::value, LAST = decltype(last)::value;
            const float kci = std::ldexp(kc, 2 * (int)i); // the colour sigma halves per iteration (its coefficient x 4)
            hipLaunchKernelGGL((k_atrous<SQUARE, LAST>), tile_grid(W, H), tile_block(), 0, st, src, alb, nrm, pos, W, H, 1 << i, kci, kni, kx, ka, dst,
                               LAST ? out_u8 : nullptr);
        });
        if (rc != RT_OK) return rc;
    }
    return end_call(d, st);
}

} // namespace

extern "C" {

int rt_denoiser_create(int device, int32_t width, int32_t height, rt_denoiser** out) {
    return rt_denoiser_create_ex(device, width, height, 0u, out);
}

int rt_denoiser_create_ex(int device, int32_t width, int32_t height, uint32_t flags, rt_denoiser** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (const int rc = image_op_check(device, width, height, flags, RT_DENOISER_VARIANCE, "unknown denoiser flag", "filter")) return rc;
    return no_throw([&]() -> int {
        rt_denoiser* d = new rt_denoiser;
        const char* oom = "hipMalloc of the denoiser's scratch and staging failed";
        int rc = image_op_open(d, device, width, height, flags, oom);
        const size_t n = d->pixels();
        if (rc == RT_OK &&
            (hipMalloc((void**)&d->d_scratch[0], n * 16u) != hipSuccess || hipMalloc((void**)&d->d_scratch[1], n * 16u) != hipSuccess ||
             ((flags & RT_DENOISER_VARIANCE) &&
              (hipMalloc((void**)&d->d_host_var_in, n * 4u) != hipSuccess || hipMalloc((void**)&d->d_host_var_out, n * 4u) != hipSuccess ||
               hipMalloc((void**)&d->d_host_mom, n * 8u) != hipSuccess || hipMalloc((void**)&d->d_host_len, n * 4u) != hipSuccess))))
            rc = fail(RT_ERR_OOM, oom);
        if (rc != RT_OK) {
            rt_denoiser_destroy(d);
            return rc;
        }
        *out = d;
        return (int)RT_OK;
    });
}

void rt_denoiser_destroy(rt_denoiser* d) {
    if (!d) return;
    if (image_op_close(d)) {
        (void)hipFree(d->d_scratch[0]), (void)hipFree(d->d_scratch[1]);
        (void)hipFree(d->d_host_var_in), (void)hipFree(d->d_host_var_out), (void)hipFree(d->d_host_mom), (void)hipFree(d->d_host_len);
    }
    delete d;
}

int rt_denoise(rt_denoiser* d, const rt_denoise_params* p, const float* rgba_f32, const float* albedo, const float* normal, const float* position,
               float* out_f32, uint8_t* out_u8) {
    if (!d || !rgba_f32 || !albedo || !normal || !position) return fail(RT_ERR_INVALID, "null argument");
    if (!out_f32 && !out_u8) return fail(RT_ERR_INVALID, "out_f32 and out_u8 are both null");
    if (const int rc = check_params(p)) return rc;
    hipStream_t st = d->stream;
    if (const int rc = stage_in(d, st, {rgba_f32, albedo, normal, position})) return rc;
    const size_t n = d->pixels();
    const float4* in = d->d_host_in;
    if (const int rc = enqueue(d, p, in, in + n, in + 2 * n, in + 3 * n, out_f32 ? d->d_host_f32 : nullptr,
                               out_u8 ? (uchar4*)d->d_host_u8 : nullptr, st))
        return rc;
    return stage_out(d, st, out_f32, out_u8);
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
