// rt_gbuffer_pixel.h — what one thread of the G-buffer kernels does: shared by k_gbuffer (rt_gbuffer.hip) and k_gbuffer_motion
// (rt_gbuffer_motion.hip). The two kernels live in units of their own: a second kernel with traversal LDS in a unit changes how the compiler
// lays out and addresses the first one's LDS (as rt_gbuffer.hip's head says of k_intersect_batch), and k_gbuffer keeps its instructions.
#pragma once
#include "rt_internal.h"
#include "rt_device.h"

namespace rt {

// One unjittered camera ray per pixel, its closest hit as k_intersect_batch finds it, then shade_hit's interpolation and normalisations
// written out with the same expressions (shade_hit itself is left alone: the render kernels' instructions must not move). Three float4
// planes, pixel i = y * W + x: albedo (scatter's attenuation, emission excluded; sky on a miss), normal (world-space shading normal, 0 on a
// miss), position (hit point, t; 0 and +inf on a miss).
// MOTION (rt_scene_gbuffer_motion): a fourth plane from the same hit, where the surface point was before the scene's last update: the hit
// triangle's PREVIOUS world-space vertices (prev_wv, 9 floats per triangle in global order: SceneUpdate::d_wv_prev) at the hit's barycentrics,
// w = 1; 0 on a miss. The flag is the presence of the two trailing arguments (prev_wv, prev_out) of gbuffer_pixel. Every kernel declares its own
// traversal LDS (RT_TRAVERSAL_LDS) and hands the stack and the staged tree top in.
RT_DEV void write_prev(uint32_t, uint32_t, float, float, float) {}
RT_DEV void write_prev(uint32_t i, uint32_t tri, float w, float bx, float by, const float* __restrict__ prev_wv, float4* __restrict__ prev_out) {
    if (tri == kNoTri) {
        prev_out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float* b = prev_wv + 9 * (size_t)tri;
    prev_out[i] = make_float4((b[0] * w + b[3] * bx) + b[6] * by, (b[1] * w + b[4] * bx) + b[7] * by, (b[2] * w + b[5] * bx) + b[8] * by, 1.0f);
}
template <typename... MOTION>
RT_DEV void gbuffer_pixel(const SceneDev& S, const CameraDev& c, const TravStack& stack, const TopTree& top, float4* __restrict__ albedo_out,
                          float4* __restrict__ normal_out, float4* __restrict__ position_out, MOTION... motion) {
    const uint32_t n = (uint32_t)c.width * (uint32_t)c.height;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % (uint32_t)c.width), y = (int)(i / (uint32_t)c.width);
    const f3 p00 = mk3(c.pixel00[0], c.pixel00[1], c.pixel00[2]);
    const f3 du = mk3(c.du[0], c.du[1], c.du[2]), dv = mk3(c.dv[0], c.dv[1], c.dv[2]);
    const f3 org = mk3(c.center[0], c.center[1], c.center[2]);
    const f3 pixel_center = (p00 + ((float)x * du)) + ((float)y * dv); // camera_ray's, without the jitter
    const f3 d = pixel_center - org;                                     // fp32: not rounded through half
    const Hit h = intersect(S, org, d, stack, top);
    if (h.tri == kNoTri) {
        albedo_out[i] = make_float4(S.sky[0], S.sky[1], S.sky[2], 0.0f);
        normal_out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        position_out[i] = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
        write_prev(i, kNoTri, 0.0f, 0.0f, 0.0f, motion...);
        return;
    }
    const ShadeRec& sr = S.shade[h.tri];
    const f3 n0 = mk3(sr.n0[0], sr.n0[1], sr.n0[2]), n1 = mk3(sr.n1[0], sr.n1[1], sr.n1[2]), n2 = mk3(sr.n2[0], sr.n2[1], sr.n2[2]);
    const uint32_t iw = sr.instance;
    const InstRec* inst = S.inst + (S.packed_mat ? (iw & kPackedInstMask) : iw);
    const MatRec& mat = S.mats[S.packed_mat ? (iw >> kPackedInstBits) : inst->material];
    const float bx = h.u, by = h.v;
    const float w = (1.0f - bx) - by;
    const float tu = (w * sr.uv0[0] + bx * sr.uv1[0]) + by * sr.uv2[0];
    const float tv = (w * sr.uv0[1] + bx * sr.uv1[1]) + by * sr.uv2[1];
    const f3 vn = normalize3((w * n0 + bx * n1) + by * n2);
    const float* nm = inst->normal_mat;
    const f3 g = mk3((nm[0] * vn.x + nm[3] * vn.y) + nm[6] * vn.z, (nm[1] * vn.x + nm[4] * vn.y) + nm[7] * vn.z,
                     (nm[2] * vn.x + nm[5] * vn.y) + nm[8] * vn.z);
    const f3 normal = normalize3(g);
    f3 a = mk3(0.0f, 0.0f, 0.0f); // RT_MAT_NONE: scatter absorbs
    if (mat.type == RT_MAT_DIFFUSE || mat.type == RT_MAT_METALLIC) a = albedo(S, mat, tu, tv);
    else if (mat.type == RT_MAT_DIELECTRIC) a = mk3(1.0f, 1.0f, 1.0f);
    albedo_out[i] = make_float4(a.x, a.y, a.z, 0.0f);
    normal_out[i] = make_float4(normal.x, normal.y, normal.z, 0.0f);
    position_out[i] = make_float4(org.x + d.x * h.t, org.y + d.y * h.t, org.z + d.z * h.t, h.t);
    write_prev(i, h.tri, w, bx, by, motion...);
}

} // namespace rt
