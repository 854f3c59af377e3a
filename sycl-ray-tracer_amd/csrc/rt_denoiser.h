// rt_denoiser.h — the denoiser's state and the small pieces its two units share: rt_denoise.hip (the a-trous filter with one global colour
// sigma) and rt_variance.hip (the variance estimate and the variance-guided filter, for a denoiser created with RT_DENOISER_VARIANCE). The
// stream protocol, the staging and the launch shape are every image op's (rt_image_op.h); the a-trous pixel and its iterations are rt_atrous_pixel.h.
#pragma once
#include "rt_image_op.h"
#include "denoise_math.h"

struct rt_denoiser : ImageOp {
    float4* d_scratch[2] = {nullptr, nullptr}; // linear colour between iterations (rt_denoise_guided: .w = the colour's variance)
    // RT_DENOISER_VARIANCE: the variance plane a host call reads, the one it writes, and rt_denoise_variance's moments and history lengths
    float* d_host_var_in = nullptr;
    float* d_host_var_out = nullptr;
    float2* d_host_mom = nullptr;
    float* d_host_len = nullptr;
};

// (an unnamed namespace in a header, on purpose: rt_denoise.hip's kernels and their table keep the symbols they had when these were its own)
namespace {

constexpr uint32_t kMaxIterations = 10;

// the weights of the B3-spline kernel, per axis: 1/16, 1/4, 3/8, 1/4, 1/16 (all exact; their products too)
__constant__ float kTapH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};

RT_DEV float dot_diff(float4 a, float4 b) { // R2's dot of a.xyz - b.xyz with itself
    const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return (x * x + y * y) + z * z;
}
RT_DEV float4 squared(float4 f) { return make_float4(f.x * f.x, f.y * f.y, f.z * f.z, 1.0f); }

} // namespace
