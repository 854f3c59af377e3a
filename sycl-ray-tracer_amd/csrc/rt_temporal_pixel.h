// rt_temporal_pixel.h — the accumulator's state, the kernels' arguments and the checks of a call: shared by k_temporal's unit (rt_temporal.hip)
// and k_temporal_moments' (rt_temporal_moments.hip). What a thread of either does is rt_temporal_pixel_body.h. The two kernels live in units of
// their own, as the G-buffer's two do (rt_gbuffer_pixel.h): k_temporal keeps its instructions, and an accumulator created without
// RT_TEMPORAL_MOMENTS never runs the other. The stream protocol, the staging and the launch shape are every image op's (rt_image_op.h); the one
// host path of a call, whichever kernel it launches, is temporal_call below.
#pragma once
#include "rt_image_op.h"

struct rt_temporal : ImageOp {
    float4* d_hist[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}}; // per set: colour (.w = history length), position, normal
    float2* d_mom[2] = {nullptr, nullptr}; // RT_TEMPORAL_MOMENTS, per set: the luminance moments (mean of l, mean of l*l)
    int cur = 0;           // the set the NEXT call writes
    bool has_prev = false; // the other set holds a frame's history (false after create / reset)
    rt_camera prev_cam{};  // ... and this was that frame's camera
    // the host variants' device copies of the history lengths and, where the accumulator has them, the moments (beside ImageOp's)
    float* d_host_len = nullptr;
    float2* d_host_mom = nullptr;
};

// (an unnamed namespace in a header, on purpose: k_temporal's symbol carries its argument's type, and it keeps the name it had when TemporalArgs
// was rt_temporal.hip's own)
namespace {

constexpr float kMinTapWeight = 0.015625f; // 1/64: a reprojection whose valid taps weigh less is no history

// What a call needs of the PREVIOUS call's camera, prepared on the host with the contract's fp32 operations (the units are compiled with
// -ffp-contract=off on both sides), and the call's thresholds.
struct TemporalArgs {
    float c[3];  // centre
    float e[3];  // pixel00 - centre
    float m[3];  // cross(du, dv): the image plane's normal
    float du[3], dv[3];
    float em;    // dot(e, m)
    float dudu, dvdv;
    float kx;         // RN(1 / RN(sigma_position^2)); 0: the position test is left out
    float cos_normal; // -1: the normal test is left out
    float max_history;
    int32_t W, H;
    uint32_t has_prev;
};

RT_DEV float dot3f(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

constexpr uint32_t kMaxHistoryLimit = 4096;

inline int check_params(const rt_temporal_params* p) {
    if (!p) return fail(RT_ERR_INVALID, "null parameters");
    if (p->max_history < 1u || p->max_history > kMaxHistoryLimit) return fail(RT_ERR_INVALID, "max_history must be 1 .. 4096");
    if (!(p->sigma_position >= kMinSigma)) return fail(RT_ERR_INVALID, "sigma_position must be at least 1e-6 (+inf switches the test off); NaN is refused");
    if (!(p->cos_normal >= -1.0f && p->cos_normal <= 1.0f)) return fail(RT_ERR_INVALID, "cos_normal must lie in [-1, 1] (-1 switches the test off); NaN is refused");
    return RT_OK;
}

inline int check_call(const rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const void* frame, const void* normal, const void* position,
                      const void* prev_position, const void* out_f32, const void* out_u8) {
    if (const int rc = check_params(p)) return rc; // (first: the parameters can be judged without an accumulator)
    if (!out_f32 && !out_u8) return fail(RT_ERR_INVALID, "out_f32 and out_u8 are both null");
    if (!t || !cam || !frame || !normal || !position || !prev_position) return fail(RT_ERR_INVALID, "null argument");
    if (cam->width != t->width || cam->height != t->height) return fail(RT_ERR_INVALID, "the camera's width and height are not the accumulator's");
    return RT_OK;
}

inline float dot3h(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the kernel's arguments of one call on `t`
inline TemporalArgs temporal_args(const rt_temporal* t, const rt_temporal_params* p) {
    TemporalArgs a{};
    const rt_camera& pc = t->prev_cam;
    for (int k = 0; k < 3; ++k) a.c[k] = pc.center[k], a.e[k] = pc.pixel00[k] - pc.center[k], a.du[k] = pc.delta_u[k], a.dv[k] = pc.delta_v[k];
    a.m[0] = a.du[1] * a.dv[2] - a.du[2] * a.dv[1];
    a.m[1] = a.du[2] * a.dv[0] - a.du[0] * a.dv[2];
    a.m[2] = a.du[0] * a.dv[1] - a.du[1] * a.dv[0];
    a.em = dot3h(a.e, a.m), a.dudu = dot3h(a.du, a.du), a.dvdv = dot3h(a.dv, a.dv);
    a.kx = coefficient(p->sigma_position), a.cos_normal = p->cos_normal, a.max_history = (float)p->max_history;
    a.W = t->width, a.H = t->height, a.has_prev = t->has_prev ? 1u : 0u;
    return a;
}

// One call on `t`, enqueued on st: the bracket, the kernel's arguments, the two sets' roles and their change. launch(a, prev, next) enqueues the
// unit's kernel under tile_grid / tile_block: it reads set prev (t->d_hist[prev], t->d_mom[prev]) and writes set next.
// PRE: the arguments were checked; all pointers are device pointers on t->device
template <typename Launch>
int temporal_call(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, hipStream_t st, Launch launch) {
    if (const int rc = begin_call(t, st)) return rc; // the previous call (any stream) is done with both sets
    launch(temporal_args(t, p), t->cur ^ 1, t->cur);
    if (const int rc = end_call(t, st)) return rc;
    t->cur ^= 1, t->has_prev = true, t->prev_cam = *cam;
    return RT_OK;
}

} // namespace

namespace rtlib {
// rt_temporal_moments.hip: rt_temporal.hip's enqueue for an accumulator that has moments (k_temporal_moments in k_temporal's place; `moments` may
// be null). PRE: the arguments were checked; all pointers are device pointers on t->device
int enqueue_temporal_moments(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const float4* frame, const float4* nrm,
                             const float4* pos, const float4* prv, float4* out_f32, uchar4* out_u8, float* hist_len, float2* moments,
                             hipStream_t st);
} // namespace rtlib
