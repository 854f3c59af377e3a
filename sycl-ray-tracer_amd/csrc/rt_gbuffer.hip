// rt_gbuffer.hip — the primary-hit G-buffer: rt_scene_gbuffer[_device] and its kernel.
// (A unit of its own, beside rt_probes.hip rather than in it: a second kernel with traversal LDS in that unit changes how the compiler lays
// out and addresses k_intersect_batch's LDS, and k_intersect_batch keeps its instructions. tests/test_denoise.py runs the ISA hazard scan of
// tests/test_isa_hazards.py on this unit's listing.)
#include "rt_internal.h"
#include "rt_device.h"

namespace rt {

// One unjittered camera ray per pixel, its closest hit as k_intersect_batch finds it, then shade_hit's interpolation and normalisations
// written out with the same expressions (shade_hit itself is left alone: the render kernels' instructions must not move). Three float4
// planes, pixel i = y * W + x: albedo (scatter's attenuation, emission excluded; sky on a miss), normal (world-space shading normal, 0 on a
// miss), position (hit point, t; 0 and +inf on a miss).
__global__ void __launch_bounds__(256) k_gbuffer(SceneDev S, CameraDev c, float4* __restrict__ albedo_out, float4* __restrict__ normal_out,
                                                  float4* __restrict__ position_out) {
    RT_TRAVERSAL_LDS(256)
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
}

} // namespace rt

namespace {

int gbuffer_check(const rt_scene* s, const rt_camera* cam) {
    if (!s || !cam) return fail(RT_ERR_INVALID, "null argument");
    if (cam->width <= 0 || cam->height <= 0) return fail(RT_ERR_INVALID, "camera width and height must be positive");
    if ((uint64_t)cam->width * (uint64_t)cam->height > 0x7fffffffull) return fail(RT_ERR_INVALID, "image too large");
    if (s->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    if (!origin_in_contract_range(s->hs, cam->center))
        return fail(RT_ERR_INVALID, "the camera lies more than 100 scene scales outside the scene's bounds: outside the range of the closest-hit contract (rt_intersect_batch)");
    return RT_OK;
}

// the launch and the event rt_scene_update waits for: one per stream, so that a launch on one stream never hides a pending one on another
// (PRE: gbuffer_check passed)
int gbuffer_enqueue(rt_scene* s, const rt_camera* cam, float4* alb, float4* nrm, float4* pos, hipStream_t st) {
    HIPCHK(hipSetDevice(s->device));
    hipEvent_t ev = nullptr;
    if (const int rc = scene_stream_event(s, st, &ev)) return rc;
    CameraDev c;
    std::memcpy(c.center, cam->center, 12), std::memcpy(c.pixel00, cam->pixel00, 12);
    std::memcpy(c.du, cam->delta_u, 12), std::memcpy(c.dv, cam->delta_v, 12);
    c.width = cam->width, c.height = cam->height;
    const uint32_t n = (uint32_t)cam->width * (uint32_t)cam->height;
    hipLaunchKernelGGL(k_gbuffer, dim3((n + 255u) / 256u), dim3(256), 0, st, s->dev, c, alb, nrm, pos);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev, st));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_scene_gbuffer(rt_scene* s, const rt_camera* cam, float* albedo, float* normal, float* position) {
    if (!albedo || !normal || !position) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = gbuffer_check(s, cam)) return rc;
    HIPCHK(hipSetDevice(s->device));
    const size_t bytes = (size_t)cam->width * (size_t)cam->height * 16u;
    DevBuf b;
    HIPCHK(b.alloc(3 * bytes));
    float4* d = b.as<float4>();
    const size_t n = bytes / 16u;
    if (const int rc = gbuffer_enqueue(s, cam, d, d + n, d + 2 * n, 0)) return rc;
    HIPCHK(hipStreamSynchronize(0));
    HIPCHK(hipMemcpy(albedo, d, bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(normal, d + n, bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(position, d + 2 * n, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_gbuffer_device(rt_scene* s, const rt_camera* cam, void* d_albedo, void* d_normal, void* d_position, void* stream) {
    if (!d_albedo || !d_normal || !d_position) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = gbuffer_check(s, cam)) return rc;
    return gbuffer_enqueue(s, cam, (float4*)d_albedo, (float4*)d_normal, (float4*)d_position, (hipStream_t)stream);
}

} // extern "C"

