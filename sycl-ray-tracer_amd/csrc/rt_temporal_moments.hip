// rt_temporal_moments.hip — k_temporal_moments, the temporal kernel that also blends the luminance moments (RT_TEMPORAL_MOMENTS), its launch (through temporal_call, as k_temporal's) and
// rt_temporal_accumulate_moments[_device]. A unit of its own for the reason rt_temporal_pixel.h gives. The contract is stated at
// rt_temporal_accumulate_moments in include/rt_mi355x.h; the numpy model that pins it bit for bit is tests/test_svgf.py: moments_model.
#include "rt_temporal_pixel.h"

namespace {

__global__ void __launch_bounds__(256) k_temporal_moments(TemporalArgs a, const float4* frame, const float4* __restrict__ nrm,
                                                           const float4* __restrict__ pos, const float4* __restrict__ prv,
                                                           const float4* __restrict__ h_col, const float4* __restrict__ h_pos,
                                                           const float4* __restrict__ h_nrm, float4* __restrict__ o_col, float4* __restrict__ o_pos,
                                                           float4* __restrict__ o_nrm, float4* out_f32, uchar4* __restrict__ out_u8,
                                                           float* __restrict__ hist_len, const float2* __restrict__ h_mom, float2* __restrict__ o_mom,
                                                           float2* __restrict__ moments) {
    constexpr bool MOMENTS = true;
#include "rt_temporal_pixel_body.h"
}

int check_moments_call(const rt_temporal* t, const void* moments) {
    if (!moments) return fail(RT_ERR_INVALID, "null argument");
    if (!(t->flags & RT_TEMPORAL_MOMENTS)) return fail(RT_ERR_INVALID, "the accumulator was created without RT_TEMPORAL_MOMENTS (rt_temporal_create_ex)");
    return RT_OK;
}

} // namespace

namespace rtlib {

int enqueue_temporal_moments(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const float4* frame, const float4* nrm,
                             const float4* pos, const float4* prv, float4* out_f32, uchar4* out_u8, float* hist_len, float2* moments,
                             hipStream_t st) {
    return temporal_call(t, p, cam, st, [&](const TemporalArgs& a, int prev, int next) {
        float4* const* h = t->d_hist[prev];
        float4* const* o = t->d_hist[next];
        hipLaunchKernelGGL(k_temporal_moments, tile_grid(a.W, a.H), tile_block(), 0, st, a, frame, nrm, pos, prv, (const float4*)h[0], (const float4*)h[1],
                           (const float4*)h[2], o[0], o[1], o[2], out_f32, out_u8, hist_len, (const float2*)t->d_mom[prev], t->d_mom[next], moments);
    });
}

} // namespace rtlib

extern "C" {

int rt_temporal_accumulate_moments(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const float* rgba_f32, const float* normal,
                                   const float* position, const float* prev_position, float* out_f32, uint8_t* out_u8, float* history_len,
                                   float* moments) {
    if (const int rc = check_call(t, p, cam, rgba_f32, normal, position, prev_position, out_f32, out_u8)) return rc;
    if (const int rc = check_moments_call(t, moments)) return rc;
    hipStream_t st = t->stream;
    if (const int rc = stage_in(t, st, {rgba_f32, normal, position, prev_position})) return rc;
    const size_t n = t->pixels();
    const float4* in = t->d_host_in;
    if (const int rc = enqueue_temporal_moments(t, p, cam, in, in + n, in + 2 * n, in + 3 * n, out_f32 ? t->d_host_f32 : nullptr,
                                                out_u8 ? (uchar4*)t->d_host_u8 : nullptr, history_len ? t->d_host_len : nullptr, t->d_host_mom, st))
        return rc;
    if (history_len) HIPCHK(hipMemcpyAsync(history_len, t->d_host_len, n * 4u, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(moments, t->d_host_mom, n * 8u, hipMemcpyDeviceToHost, st));
    return stage_out(t, st, out_f32, out_u8);
}

int rt_temporal_accumulate_moments_device(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const void* d_rgba_f32,
                                          const void* d_normal, const void* d_position, const void* d_prev_position, void* d_out_f32, void* d_out_u8,
                                          void* d_history_len, void* d_moments, void* stream) {
    if (const int rc = check_call(t, p, cam, d_rgba_f32, d_normal, d_position, d_prev_position, d_out_f32, d_out_u8)) return rc;
    if (const int rc = check_moments_call(t, d_moments)) return rc;
    return enqueue_temporal_moments(t, p, cam, (const float4*)d_rgba_f32, (const float4*)d_normal, (const float4*)d_position,
                                    (const float4*)d_prev_position, (float4*)d_out_f32, (uchar4*)d_out_u8, (float*)d_history_len,
                                    (float2*)d_moments, (hipStream_t)stream);
}

} // extern "C"
