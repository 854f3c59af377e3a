// rt_image_op.h — what the image-space passes share: the denoiser (rt_denoise.hip, rt_variance.hip) and the temporal accumulator (rt_temporal.hip,
// rt_temporal_moments.hip). An image op is an object for W x H frames on one device with a stream of its own for its host entry points, staging
// planes for their arguments, and the bracket every call goes through (CallBracket, rt_internal.h): the next call, on whatever stream, waits for
// the last before it touches the planes the object owns (scratch, history sets, staging).
#pragma once
#include "rt_internal.h"
#include "rt_device.h"

struct ImageOp : CallBracket {
    int32_t width = 0, height = 0;
    uint32_t flags = 0; // RT_DENOISER_* / RT_TEMPORAL_*
    // the host entry points' device copies of their arguments (four 16-byte input planes, the fp32 and unorm8 outputs), allocated at creation: no
    // call allocates
    float4* d_host_in = nullptr;
    float4* d_host_f32 = nullptr;
    uint8_t* d_host_u8 = nullptr;
    size_t pixels() const { return (size_t)width * (size_t)height; }
};

// (an unnamed namespace in a header, on purpose, as rt_denoiser.h's and rt_temporal_pixel.h's: the kernels of the units that include this keep
// the symbols and the instructions they had when these were the units' own)
namespace {

constexpr float kMinSigma = 1e-6f;

// RN(1 / RN(sigma * sigma)); 0 for sigma = +inf (the guide ignored, the test left out)
inline float coefficient(float sigma) {
    if (std::isinf(sigma)) return 0.0f;
    const float s2 = sigma * sigma;
    return 1.0f / s2;
}

// The launch shape of every per-pixel kernel here: a 1-D grid of 64 x 4 tiles, row-major (a second grid dimension would bound the image's
// height); a workgroup is one tile, a wave one row of 64 consecutive pixels. W * H < 2^31 and the grid's threads < 2^32 (image_op_check): the
// tile count and every thread index fit in 32 bits.
inline dim3 tile_grid(int32_t W, int32_t H) { return dim3((((uint32_t)W + 63u) / 64u) * (((uint32_t)H + 3u) / 4u)); }
inline dim3 tile_block() { return dim3(64, 4); }

// the thread's pixel under that shape; false: outside the image (the temporal body, rt_temporal_pixel_body.h, keeps these lines as its own text)
RT_DEV bool tile_pixel(int32_t W, int32_t H, int32_t* x, int32_t* y) {
    const uint32_t tiles_x = ((uint32_t)W + 63u) / 64u;
    *x = (int32_t)((blockIdx.x % tiles_x) * 64u + threadIdx.x), *y = (int32_t)((blockIdx.x / tiles_x) * 4u + threadIdx.y);
    return *x < W && *y < H;
}

} // namespace

namespace rtlib {

// The refusals of a creation, in their order. flag_msg: the object's wording of an unknown flag; grid_owner: whose launch grid the shape has to fit
// ("filter", "kernel"). The device is current where this returns RT_OK.
inline int image_op_check(int device, int32_t width, int32_t height, uint32_t flags, uint32_t known_flags, const char* flag_msg, const char* grid_owner) {
    if (device < 0) return fail(RT_ERR_INVALID, "device index out of range");
    if (flags & ~known_flags) return fail(RT_ERR_INVALID, flag_msg);
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "width and height must be positive");
    if ((uint64_t)width * (uint64_t)height > 0x7fffffffull) return fail(RT_ERR_INVALID, "image too large (W x H must stay below 2^31)");
    // tile_grid's threads, padding included, must stay below 2^32 (only very narrow images reach that)
    if (((uint64_t)width + 63u) / 64u * (((uint64_t)height + 3u) / 4u) * 256u > 0xffffffffull)
        return fail(RT_ERR_INVALID, std::string("image shape too narrow and tall for the ") + grid_owner + "'s launch grid");
    return device_ok(device);
}

// fills the shared members of a new object (PRE: image_op_check passed). oom_msg: the object's wording of a failed hipMalloc, its own planes'
// too. Whatever this returns, image_op_close releases what was made.
inline int image_op_open(ImageOp* op, int device, int32_t width, int32_t height, uint32_t flags, const char* oom_msg) {
    op->device = device, op->width = width, op->height = height, op->flags = flags;
    const size_t n = op->pixels();
    if (hipMalloc((void**)&op->d_host_in, 4 * n * 16u) != hipSuccess || hipMalloc((void**)&op->d_host_f32, n * 16u) != hipSuccess ||
        hipMalloc((void**)&op->d_host_u8, n * 4u) != hipSuccess)
        return fail(RT_ERR_OOM, oom_msg);
    return bracket_open(op);
}

// waits for the last call and releases the shared members; true: the device is current and the caller frees its own planes
inline bool image_op_close(ImageOp* op) {
    if (!bracket_close(op)) return false;
    (void)hipFree(op->d_host_in), (void)hipFree(op->d_host_f32), (void)hipFree(op->d_host_u8);
    return true;
}

// the four 16-byte input planes of a host call -> d_host_in, plane k at d_host_in + k * pixels() (behind the wait: a _device call may still read them)
inline int stage_in(ImageOp* op, hipStream_t st, const float* const (&planes)[4]) {
    if (const int rc = begin_call(op, st)) return rc;
    const size_t n = op->pixels();
    for (int k = 0; k < 4; ++k) HIPCHK(hipMemcpyAsync(op->d_host_in + k * n, planes[k], n * 16u, hipMemcpyHostToDevice, st));
    return RT_OK;
}
// d_host_f32 and d_host_u8 -> the host call's outputs (each may be null), then the call's end: the stream has run dry
inline int stage_out(ImageOp* op, hipStream_t st, float* out_f32, uint8_t* out_u8) {
    const size_t n = op->pixels();
    if (out_f32) HIPCHK(hipMemcpyAsync(out_f32, op->d_host_f32, n * 16u, hipMemcpyDeviceToHost, st));
    if (out_u8) HIPCHK(hipMemcpyAsync(out_u8, op->d_host_u8, n * 4u, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

} // namespace rtlib
