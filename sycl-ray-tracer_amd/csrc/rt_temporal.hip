// rt_temporal.hip — temporal accumulation by reprojection: rt_temporal_create / _destroy / _reset, rt_temporal_accumulate[_device] and their
// kernel. The arithmetic is the contract stated at rt_temporal_accumulate in include/rt_mi355x.h; the numpy model that pins it bit for bit is
// tests/test_temporal.py: temporal_model.
//
// One launch per call. The accumulator owns two sets of three float4 planes (history colour with the history length in .w, and the position
// and normal planes of the frame that history belongs to): a call reads the previous set through its four bilinear taps and writes the
// current one, then the two change roles. A workgroup is 64 x 4 pixels, a wave one row of 64 consecutive pixels: every plane load and store
// of a wave is one contiguous 1 KB row segment, and the taps of a wave land on neighbouring pixels of the previous set for any coherent
// motion. No atomics, no grid synchronisation: the kernel boundary is the only hand-off.
#include "rt_internal.h"
#include "rt_device.h"

struct rt_temporal {
    int device = -1;
    int32_t width = 0, height = 0;
    float4* d_hist[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}}; // per set: colour (.w = history length), position, normal
    int cur = 0;           // the set the NEXT call writes
    bool has_prev = false; // the other set holds a frame's history (false after create / reset)
    rt_camera prev_cam{};  // ... and this was that frame's camera
    hipStream_t stream = nullptr; // rt_temporal_accumulate (the host variant) runs here
    hipEvent_t ev_last = nullptr; // recorded behind every call: the next call's stream waits for it
    bool recorded = false;
    // rt_temporal_accumulate's device copies of its host arguments (four input planes, the fp32 and unorm8 outputs, the history lengths),
    // allocated with the sets at creation: no call allocates
    float4* d_host_in = nullptr;
    float4* d_host_f32 = nullptr;
    uint8_t* d_host_u8 = nullptr;
    float* d_host_len = nullptr;
};

namespace {

constexpr uint32_t kMaxHistoryLimit = 4096;
constexpr float kMinSigma = 1e-6f;
constexpr float kMinTapWeight = 0.015625f; // 1/64: a reprojection whose valid taps weigh less is no history

// What a call needs of the PREVIOUS call's camera, prepared on the host with the contract's fp32 operations (this unit is compiled with
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

__global__ void __launch_bounds__(256) k_temporal(TemporalArgs a, const float4* frame, const float4* __restrict__ nrm, const float4* __restrict__ pos,
                                                   const float4* __restrict__ prv, const float4* __restrict__ h_col, const float4* __restrict__ h_pos,
                                                   const float4* __restrict__ h_nrm, float4* __restrict__ o_col, float4* __restrict__ o_pos,
                                                   float4* __restrict__ o_nrm, float4* out_f32, uchar4* __restrict__ out_u8,
                                                   float* __restrict__ hist_len) {
    // a 1-D grid of 64 x 4 tiles, row-major (as k_atrous)
    const int32_t W = a.W, H = a.H;
    const uint32_t tiles_x = ((uint32_t)W + 63u) / 64u;
    const int32_t x = (int32_t)((blockIdx.x % tiles_x) * 64u + threadIdx.x), y = (int32_t)((blockIdx.x / tiles_x) * 4u + threadIdx.y);
    if (x >= W || y >= H) return;
    const int32_t p = y * W + x;
    const float4 F = frame[p], N = nrm[p], P = pos[p];
    const bool hit = __builtin_isfinite(P.w);
    const float lx = F.x * F.x, ly = F.y * F.y, lz = F.z * F.z;
    float ox = lx, oy = ly, oz = lz, n_new = hit ? 1.0f : 0.0f;
    bool blended = false;
    if (a.has_prev && hit) {
        const float4 Q = prv[p];
        const float rx = Q.x - a.c[0], ry = Q.y - a.c[1], rz = Q.z - a.c[2];
        const float s = a.em / dot3f(rx, ry, rz, a.m[0], a.m[1], a.m[2]);
        if (__builtin_isfinite(s) && s > 0.0f) {
            const float hx = rx * s - a.e[0], hy = ry * s - a.e[1], hz = rz * s - a.e[2];
            const float sx = dot3f(hx, hy, hz, a.du[0], a.du[1], a.du[2]) / a.dudu;
            const float sy = dot3f(hx, hy, hz, a.dv[0], a.dv[1], a.dv[2]) / a.dvdv;
            if (sx > -1.0f && sx < (float)W && sy > -1.0f && sy < (float)H) { // (NaN fails here, before any conversion to an integer)
                const float x0f = __builtin_floorf(sx), y0f = __builtin_floorf(sy);
                const float fx = sx - x0f, fy = sy - y0f;
                const float gx = 1.0f - fx, gy = 1.0f - fy;
                const int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;
                // The four taps' guides are fetched at once, from addresses clamped into the image (a tap outside it is dropped below): four
                // independent loads per plane in flight instead of a chain of dependent ones. The colour is read only where the guides passed.
                int32_t q[4];
                float w[4];
                bool valid[4];
                float4 Pt[4], Nt[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = k & 1, j = k >> 1; // tap order (0,0), (1,0), (0,1), (1,1)
                    const int32_t tx = x0 + i, ty = y0 + j;
                    w[k] = (i ? fx : gx) * (j ? fy : gy);
                    valid[k] = tx >= 0 && tx < W && ty >= 0 && ty < H && w[k] > 0.0f;
                    q[k] = min(max(ty, 0), H - 1) * W + min(max(tx, 0), W - 1);
                    Pt[k] = h_pos[q[k]];
                }
                if (a.cos_normal != -1.0f) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) Nt[k] = h_nrm[q[k]];
                }
                float wsum = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, n_min = __builtin_inff();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    bool ok = valid[k] && __builtin_isfinite(Pt[k].w); // (a miss of the previous frame: its stored length is 0)
                    if (a.kx != 0.0f) {
                        const float dx = Pt[k].x - Q.x, dy = Pt[k].y - Q.y, dz = Pt[k].z - Q.z;
                        ok = ok && dot3f(dx, dy, dz, dx, dy, dz) * a.kx <= 1.0f;
                    }
                    if (a.cos_normal != -1.0f) ok = ok && dot3f(N.x, N.y, N.z, Nt[k].x, Nt[k].y, Nt[k].z) >= a.cos_normal;
                    valid[k] = ok;
                }
                float4 Ct[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (valid[k]) Ct[k] = h_col[q[k]];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!valid[k]) continue;
                    wsum = wsum + w[k];
                    sr = sr + w[k] * Ct[k].x, sg = sg + w[k] * Ct[k].y, sb = sb + w[k] * Ct[k].z;
                    n_min = __builtin_fminf(n_min, Ct[k].w);
                }
                if (wsum >= kMinTapWeight) {
                    const float n_next = __builtin_fminf(n_min + 1.0f, a.max_history);
                    if (n_next != 1.0f) {
                        const float hr = sr / wsum, hg = sg / wsum, hb = sb / wsum;
                        const float alpha = 1.0f / n_next;
                        ox = hr + (lx - hr) * alpha, oy = hg + (ly - hg) * alpha, oz = hb + (lz - hb) * alpha;
                        n_new = n_next;
                        blended = true;
                    }
                }
            }
        }
    }
    o_col[p] = make_float4(ox, oy, oz, n_new);
    o_pos[p] = P;
    o_nrm[p] = N;
    // without history the outputs are the input's own values, not the square root of their squares
    const float fr = blended ? __builtin_sqrtf(ox) : F.x, fg = blended ? __builtin_sqrtf(oy) : F.y, fb = blended ? __builtin_sqrtf(oz) : F.z;
    if (out_f32) out_f32[p] = make_float4(fr, fg, fb, 1.0f);
    if (out_u8) out_u8[p] = make_uchar4(to_unorm8(fr), to_unorm8(fg), to_unorm8(fb), 255);
    if (hist_len) hist_len[p] = n_new;
}

// RN(1 / RN(sigma * sigma)); 0 for sigma = +inf (the test left out): the denoiser's coefficient()
float coefficient(float sigma) {
    if (std::isinf(sigma)) return 0.0f;
    const float s2 = sigma * sigma;
    return 1.0f / s2;
}

int check_params(const rt_temporal_params* p) {
    if (!p) return fail(RT_ERR_INVALID, "null parameters");
    if (p->max_history < 1u || p->max_history > kMaxHistoryLimit) return fail(RT_ERR_INVALID, "max_history must be 1 .. 4096");
    if (!(p->sigma_position >= kMinSigma)) return fail(RT_ERR_INVALID, "sigma_position must be at least 1e-6 (+inf switches the test off); NaN is refused");
    if (!(p->cos_normal >= -1.0f && p->cos_normal <= 1.0f)) return fail(RT_ERR_INVALID, "cos_normal must lie in [-1, 1] (-1 switches the test off); NaN is refused");
    return RT_OK;
}

int check_call(const rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const void* frame, const void* normal, const void* position,
               const void* prev_position, const void* out_f32, const void* out_u8) {
    if (const int rc = check_params(p)) return rc; // (first: the parameters can be judged without an accumulator)
    if (!out_f32 && !out_u8) return fail(RT_ERR_INVALID, "out_f32 and out_u8 are both null");
    if (!t || !cam || !frame || !normal || !position || !prev_position) return fail(RT_ERR_INVALID, "null argument");
    if (cam->width != t->width || cam->height != t->height) return fail(RT_ERR_INVALID, "the camera's width and height are not the accumulator's");
    return RT_OK;
}

float dot3h(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// PRE: the arguments were checked; all pointers are device pointers on t->device
int enqueue(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const float4* frame, const float4* nrm, const float4* pos,
            const float4* prv, float4* out_f32, uchar4* out_u8, float* hist_len, hipStream_t st) {
    HIPCHK(hipSetDevice(t->device));
    if (t->recorded) HIPCHK(hipStreamWaitEvent(st, t->ev_last, 0)); // the previous call (any stream) is done with both sets
    TemporalArgs a{};
    const rt_camera& pc = t->prev_cam;
    for (int k = 0; k < 3; ++k) a.c[k] = pc.center[k], a.e[k] = pc.pixel00[k] - pc.center[k], a.du[k] = pc.delta_u[k], a.dv[k] = pc.delta_v[k];
    a.m[0] = a.du[1] * a.dv[2] - a.du[2] * a.dv[1];
    a.m[1] = a.du[2] * a.dv[0] - a.du[0] * a.dv[2];
    a.m[2] = a.du[0] * a.dv[1] - a.du[1] * a.dv[0];
    a.em = dot3h(a.e, a.m), a.dudu = dot3h(a.du, a.du), a.dvdv = dot3h(a.dv, a.dv);
    a.kx = coefficient(p->sigma_position), a.cos_normal = p->cos_normal, a.max_history = (float)p->max_history;
    a.W = t->width, a.H = t->height, a.has_prev = t->has_prev ? 1u : 0u;
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
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (device < 0) return fail(RT_ERR_INVALID, "device index out of range");
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "width and height must be positive");
    if ((uint64_t)width * (uint64_t)height > 0x7fffffffull) return fail(RT_ERR_INVALID, "image too large (W x H must stay below 2^31)");
    // k_temporal's 1-D grid of 64 x 4 tiles: its threads, padding included, must stay below 2^32 (only very narrow images reach that)
    if (((uint64_t)width + 63u) / 64u * (((uint64_t)height + 3u) / 4u) * 256u > 0xffffffffull)
        return fail(RT_ERR_INVALID, "image shape too narrow and tall for the kernel's launch grid");
    const int rc = device_ok(device);
    if (rc != RT_OK) return rc;
    return no_throw([&]() -> int {
        rt_temporal* t = new rt_temporal;
        t->device = device, t->width = width, t->height = height;
        const size_t n = (size_t)width * (size_t)height, bytes = n * 16u;
        bool ok = true;
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k) ok = ok && hipMalloc((void**)&t->d_hist[s][k], bytes) == hipSuccess;
        ok = ok && hipMalloc((void**)&t->d_host_in, 4 * bytes) == hipSuccess && hipMalloc((void**)&t->d_host_f32, bytes) == hipSuccess &&
             hipMalloc((void**)&t->d_host_u8, n * 4u) == hipSuccess && hipMalloc((void**)&t->d_host_len, n * 4u) == hipSuccess;
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
