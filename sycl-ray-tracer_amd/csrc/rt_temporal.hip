// rt_temporal.hip — temporal accumulation by reprojection: rt_temporal_create[_ex] / _destroy / _reset, rt_temporal_accumulate[_device] and their
// kernel (what a thread does: rt_temporal_pixel.h; the variant that also carries luminance moments: rt_temporal_moments.hip). The arithmetic is the contract stated at rt_temporal_accumulate in include/rt_mi355x.h; the numpy model that pins it bit for bit is
// tests/test_temporal.py: temporal_model.
//
// One launch per call. The accumulator owns two sets of three float4 planes (history colour with the history length in .w, and the position
// and normal planes of the frame that history belongs to): a call reads the previous set through its four bilinear taps and writes the
// current one, then the two change roles. A workgroup is 64 x 4 pixels, a wave one row of 64 consecutive pixels: every plane load and store
// of a wave is one contiguous 1 KB row segment, and the taps of a wave land on neighbouring pixels of the previous set for any coherent
// motion. No atomics, no grid synchronisation: the kernel boundary is the only hand-off. The host path of a call is
// rt_temporal_pixel.h: temporal_call, shared with rt_temporal_moments.hip; creation, the bracket and the host staging are rt_image_op.h's.
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
    return temporal_call(t, p, cam, st, [&](const TemporalArgs& a, int prev, int next) {
        float4* const* h = t->d_hist[prev];
        float4* const* o = t->d_hist[next];
        hipLaunchKernelGGL(k_temporal, tile_grid(a.W, a.H), tile_block(), 0, st, a, frame, nrm, pos, prv, (const float4*)h[0], (const float4*)h[1],
                           (const float4*)h[2], o[0], o[1], o[2], out_f32, out_u8, hist_len);
    });
}

} // namespace

extern "C" {

int rt_temporal_create(int device, int32_t width, int32_t height, rt_temporal** out) {
    return rt_temporal_create_ex(device, width, height, 0u, out);
}

int rt_temporal_create_ex(int device, int32_t width, int32_t height, uint32_t flags, rt_temporal** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (const int rc = image_op_check(device, width, height, flags, RT_TEMPORAL_MOMENTS, "unknown accumulator flag", "kernel")) return rc;
    return no_throw([&]() -> int {
        rt_temporal* t = new rt_temporal;
        const char* oom = "hipMalloc of the accumulator's history and staging failed";
        int rc = image_op_open(t, device, width, height, flags, oom);
        const size_t n = t->pixels();
        bool ok = rc == RT_OK;
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k) ok = ok && hipMalloc((void**)&t->d_hist[s][k], n * 16u) == hipSuccess;
        ok = ok && hipMalloc((void**)&t->d_host_len, n * 4u) == hipSuccess;
        if (flags & RT_TEMPORAL_MOMENTS)
            ok = ok && hipMalloc((void**)&t->d_mom[0], n * 8u) == hipSuccess && hipMalloc((void**)&t->d_mom[1], n * 8u) == hipSuccess &&
                 hipMalloc((void**)&t->d_host_mom, n * 8u) == hipSuccess;
        if (rc == RT_OK && !ok) rc = fail(RT_ERR_OOM, oom);
        if (rc != RT_OK) {
            rt_temporal_destroy(t);
            return rc;
        }
        *out = t;
        return (int)RT_OK;
    });
}

void rt_temporal_destroy(rt_temporal* t) {
    if (!t) return;
    if (image_op_close(t)) {
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k) (void)hipFree(t->d_hist[s][k]);
        (void)hipFree(t->d_host_len), (void)hipFree(t->d_mom[0]), (void)hipFree(t->d_mom[1]), (void)hipFree(t->d_host_mom);
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
    hipStream_t st = t->stream;
    if (const int rc = stage_in(t, st, {rgba_f32, normal, position, prev_position})) return rc;
    const size_t n = t->pixels();
    const float4* in = t->d_host_in;
    if (const int rc = enqueue(t, p, cam, in, in + n, in + 2 * n, in + 3 * n, out_f32 ? t->d_host_f32 : nullptr,
                               out_u8 ? (uchar4*)t->d_host_u8 : nullptr, history_len ? t->d_host_len : nullptr, st))
        return rc;
    if (history_len) HIPCHK(hipMemcpyAsync(history_len, t->d_host_len, n * 4u, hipMemcpyDeviceToHost, st));
    return stage_out(t, st, out_f32, out_u8);
}

int rt_temporal_accumulate_device(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const void* d_rgba_f32, const void* d_normal,
                                  const void* d_position, const void* d_prev_position, void* d_out_f32, void* d_out_u8, void* d_history_len,
                                  void* stream) {
    if (const int rc = check_call(t, p, cam, d_rgba_f32, d_normal, d_position, d_prev_position, d_out_f32, d_out_u8)) return rc;
    return enqueue(t, p, cam, (const float4*)d_rgba_f32, (const float4*)d_normal, (const float4*)d_position, (const float4*)d_prev_position,
                   (float4*)d_out_f32, (uchar4*)d_out_u8, (float*)d_history_len, (hipStream_t)stream);
}

} // extern "C"
