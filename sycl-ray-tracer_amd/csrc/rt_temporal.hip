// rt_temporal.hip — temporal accumulation by reprojection: rt_temporal_create[_ex] / _destroy / _reset, rt_temporal_accumulate[_device] and their
// kernel (what a thread does: rt_temporal_pixel.h; the variant that also carries luminance moments: rt_temporal_moments.hip). The arithmetic is the contract stated at rt_temporal_accumulate in include/rt_mi355x.h; the numpy model that pins it bit for bit is
// tests/test_temporal.py: temporal_model.
//
// One launch per call. The accumulator owns two sets of three float4 planes (history colour with the history length in .w, and the position
// and normal planes of the frame that history belongs to): a call reads the previous set through its four bilinear taps and writes the
// current one, then the two change roles. A workgroup is 64 x 4 pixels, a wave one row of 64 consecutive pixels: every plane load and store
// of a wave is one contiguous 1 KB row segment, and the taps of a wave land on neighbouring pixels of the previous set for any coherent
// motion. No atomics, no grid synchronisation: the kernel boundary is the only hand-off.
#include "rt_temporal_pixel.h"

namespace {

__global__ void __launch_bounds__(256) k_temporal(TemporalArgs a, const float4* frame, const float4* __restrict__ nrm, const float4* __restrict__ pos,
                                                   const float4* __restrict__ prv, const float4* __restrict__ h_col, const float4* __restrict__ h_pos,
                                                   const float4* __restrict__ h_nrm, float4* __restrict__ o_col, float4* __restrict__ o_pos,
                                                   float4* __restrict__ o_nrm, float4* out_f32, uchar4* __restrict__ out_u8,
                                                   float* __restrict__ hist_len) {
    constexpr bool MOMENTS = false;
    constexpr float2* h_mom = nullptr; // (named in the body's discarded branches only)
    constexpr float2* o_mom = nullptr;
    constexpr float2* moments = nullptr;
#include "rt_temporal_pixel_body.h"
}

// PRE: the arguments were checked; all pointers are device pointers on t->device
int enqueue(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const float4* frame, const float4* nrm, const float4* pos,
            const float4* prv, float4* out_f32, uchar4* out_u8, float* hist_len, hipStream_t st) {
    // an accumulator that has moments keeps them up to date through plain calls too: the same colour, from the kernel that also blends the moments
    if (t->flags & RT_TEMPORAL_MOMENTS) return enqueue_temporal_moments(t, p, cam, frame, nrm, pos, prv, out_f32, out_u8, hist_len, nullptr, st);
    HIPCHK(hipSetDevice(t->device));
    if (t->recorded) HIPCHK(hipStreamWaitEvent(st, t->ev_last, 0)); // the previous call (any stream) is done with both sets
    const TemporalArgs a = temporal_args(t, p);
    float4* const* prev = t->d_hist[t->cur ^ 1];
    float4* const* next = t->d_hist[t->cur];
    // W * H < 2^31 and the grid's threads < 2^32 (rt_temporal_create): every index fits in 32 bits
    const dim3 grid((((uint32_t)a.W + 63u) / 64u) * (((uint32_t)a.H + 3u) / 4u)), block(64, 4);
    hipLaunchKernelGGL(k_temporal, grid, block, 0, st, a, frame, nrm, pos, prv, (const float4*)prev[0], (const float4*)prev[1], (const float4*)prev[2],
                       next[0], next[1], next[2], out_f32, out_u8, hist_len);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(t->ev_last, st));
    t->recorded = true;
    t->cur ^= 1, t->has_prev = true, t->prev_cam = *cam;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_temporal_create(int device, int32_t width, int32_t height, rt_temporal** out) {
    return rt_temporal_create_ex(device, width, height, 0u, out);
}

int rt_temporal_create_ex(int device, int32_t width, int32_t height, uint32_t flags, rt_temporal** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (device < 0) return fail(RT_ERR_INVALID, "device index out of range");
    if (flags & ~RT_TEMPORAL_MOMENTS) return fail(RT_ERR_INVALID, "unknown accumulator flag");
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "width and height must be positive");
    if ((uint64_t)width * (uint64_t)height > 0x7fffffffull) return fail(RT_ERR_INVALID, "image too large (W x H must stay below 2^31)");
    // k_temporal's 1-D grid of 64 x 4 tiles: its threads, padding included, must stay below 2^32 (only very narrow images reach that)
    if (((uint64_t)width + 63u) / 64u * (((uint64_t)height + 3u) / 4u) * 256u > 0xffffffffull)
        return fail(RT_ERR_INVALID, "image shape too narrow and tall for the kernel's launch grid");
    const int rc = device_ok(device);
    if (rc != RT_OK) return rc;
    return no_throw([&]() -> int {
        rt_temporal* t = new rt_temporal;
        t->device = device, t->width = width, t->height = height, t->flags = flags;
        const size_t n = (size_t)width * (size_t)height, bytes = n * 16u;
        bool ok = true;
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k) ok = ok && hipMalloc((void**)&t->d_hist[s][k], bytes) == hipSuccess;
        ok = ok && hipMalloc((void**)&t->d_host_in, 4 * bytes) == hipSuccess && hipMalloc((void**)&t->d_host_f32, bytes) == hipSuccess &&
             hipMalloc((void**)&t->d_host_u8, n * 4u) == hipSuccess && hipMalloc((void**)&t->d_host_len, n * 4u) == hipSuccess;
        if (flags & RT_TEMPORAL_MOMENTS)
            ok = ok && hipMalloc((void**)&t->d_mom[0], n * 8u) == hipSuccess && hipMalloc((void**)&t->d_mom[1], n * 8u) == hipSuccess &&
                 hipMalloc((void**)&t->d_host_mom, n * 8u) == hipSuccess;
        if (!ok) {
            rt_temporal_destroy(t);
            return fail(RT_ERR_OOM, "hipMalloc of the accumulator's history and staging failed");
        }
        if (hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&t->ev_last, hipEventDisableTiming) != hipSuccess) {
            rt_temporal_destroy(t);
            return fail(RT_ERR_HIP, "hipStreamCreate / hipEventCreate failed");
        }
        *out = t;
        return (int)RT_OK;
    });
}

void rt_temporal_destroy(rt_temporal* t) {
    if (!t) return;
    if (t->device >= 0 && hipSetDevice(t->device) == hipSuccess) {
        if (t->recorded) (void)hipEventSynchronize(t->ev_last);
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k) (void)hipFree(t->d_hist[s][k]);
        (void)hipFree(t->d_host_in), (void)hipFree(t->d_host_f32), (void)hipFree(t->d_host_u8), (void)hipFree(t->d_host_len);
        (void)hipFree(t->d_mom[0]), (void)hipFree(t->d_mom[1]), (void)hipFree(t->d_host_mom);
        if (t->ev_last) (void)hipEventDestroy(t->ev_last);
        if (t->stream) (void)hipStreamDestroy(t->stream);
    }
    delete t;
}

int rt_temporal_reset(rt_temporal* t) {
    if (!t) return fail(RT_ERR_INVALID, "null accumulator");
    t->has_prev = false; // (host state only: whether the kernel looks at the previous set is an argument of the next launch)
    return RT_OK;
}

int rt_temporal_accumulate(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const float* rgba_f32, const float* normal,
                           const float* position, const float* prev_position, float* out_f32, uint8_t* out_u8, float* history_len) {
    if (const int rc = check_call(t, p, cam, rgba_f32, normal, position, prev_position, out_f32, out_u8)) return rc;
    HIPCHK(hipSetDevice(t->device));
    const size_t n = (size_t)t->width * (size_t)t->height, bytes = n * 16u;
    float4* in = t->d_host_in;
    hipStream_t st = t->stream;
    if (t->recorded) HIPCHK(hipStreamWaitEvent(st, t->ev_last, 0)); // a _device call on another stream may still run
    HIPCHK(hipMemcpyAsync(in, rgba_f32, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + n, normal, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + 2 * n, position, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(in + 3 * n, prev_position, bytes, hipMemcpyHostToDevice, st));
    if (const int rc = enqueue(t, p, cam, in, in + n, in + 2 * n, in + 3 * n, out_f32 ? t->d_host_f32 : nullptr,
                               out_u8 ? (uchar4*)t->d_host_u8 : nullptr, history_len ? t->d_host_len : nullptr, st))
        return rc;
    if (out_f32) HIPCHK(hipMemcpyAsync(out_f32, t->d_host_f32, bytes, hipMemcpyDeviceToHost, st));
    if (out_u8) HIPCHK(hipMemcpyAsync(out_u8, t->d_host_u8, n * 4u, hipMemcpyDeviceToHost, st));
    if (history_len) HIPCHK(hipMemcpyAsync(history_len, t->d_host_len, n * 4u, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_temporal_accumulate_device(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const void* d_rgba_f32, const void* d_normal,
                                  const void* d_position, const void* d_prev_position, void* d_out_f32, void* d_out_u8, void* d_history_len,
                                  void* stream) {
    if (const int rc = check_call(t, p, cam, d_rgba_f32, d_normal, d_position, d_prev_position, d_out_f32, d_out_u8)) return rc;
    return enqueue(t, p, cam, (const float4*)d_rgba_f32, (const float4*)d_normal, (const float4*)d_position, (const float4*)d_prev_position,
                   (float4*)d_out_f32, (uchar4*)d_out_u8, (float*)d_history_len, (hipStream_t)stream);
}

} // extern "C"
