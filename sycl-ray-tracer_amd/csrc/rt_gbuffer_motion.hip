// rt_gbuffer_motion.hip — k_gbuffer_motion, the G-buffer kernel that also writes the motion guide (rt_scene_gbuffer_motion[_device]: the entry
// points are in rt_gbuffer.hip), and its launch. A unit of its own for the reason rt_gbuffer_pixel.h gives.
#include "rt_gbuffer_pixel.h"

namespace rt {

__global__ void __launch_bounds__(256) k_gbuffer_motion(SceneDev S, CameraDev c, float4* __restrict__ albedo_out, float4* __restrict__ normal_out,
                                                         float4* __restrict__ position_out, const float* __restrict__ prev_wv,
                                                         float4* __restrict__ prev_out) {
    RT_TRAVERSAL_LDS(256)
    gbuffer_pixel(S, c, stack, top, albedo_out, normal_out, position_out, prev_wv, prev_out);
}

} // namespace rt

namespace rtlib {
void launch_gbuffer_motion(const SceneDev& S, const CameraDev& c, uint32_t n, float4* alb, float4* nrm, float4* pos, const float* prev_wv, float4* prev,
                           hipStream_t st) {
    hipLaunchKernelGGL(k_gbuffer_motion, dim3((n + 255u) / 256u), dim3(256), 0, st, S, c, alb, nrm, pos, prev_wv, prev);
}
} // namespace rtlib
