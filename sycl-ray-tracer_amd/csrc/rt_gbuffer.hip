// rt_gbuffer.hip — the primary-hit G-buffer: rt_scene_gbuffer[_device], rt_scene_gbuffer_motion[_device] and k_gbuffer (k_gbuffer_motion: rt_gbuffer_motion.hip).
// (A unit of its own, beside rt_probes.hip rather than in it: a second kernel with traversal LDS in that unit changes how the compiler lays
// out and addresses k_intersect_batch's LDS, and k_intersect_batch keeps its instructions. tests/test_denoise.py runs the ISA hazard scan of
// tests/test_isa_hazards.py on this unit's listing.)
#include "rt_gbuffer_pixel.h"

namespace rt {

__global__ void __launch_bounds__(256) k_gbuffer(SceneDev S, CameraDev c, float4* __restrict__ albedo_out, float4* __restrict__ normal_out,
                                                  float4* __restrict__ position_out) {
    RT_TRAVERSAL_LDS(256)
    gbuffer_pixel(S, c, stack, top, albedo_out, normal_out, position_out);
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

// rt_scene_gbuffer_motion: the scene keeps its previous vertices (PRE: gbuffer_check passed)
int motion_check(const rt_scene* s) {
    if (!s->upd || !s->upd->keep_previous) return fail(RT_ERR_INVALID, "the scene does not keep its previous vertices (rt_scene_create_ex with RT_SCENE_KEEP_PREVIOUS | RT_SCENE_UPDATABLE)");
    return RT_OK;
}

// the launch and the event rt_scene_update waits for: one per stream, so that a launch on one stream never hides a pending one on another
// (PRE: gbuffer_check passed)
int gbuffer_enqueue(rt_scene* s, const rt_camera* cam, float4* alb, float4* nrm, float4* pos, float4* prev, hipStream_t st) {
    HIPCHK(hipSetDevice(s->device));
    hipEvent_t ev = nullptr;
    if (const int rc = scene_stream_event(s, st, &ev)) return rc;
    const CameraDev c = to_dev(*cam);
    const uint32_t n = (uint32_t)cam->width * (uint32_t)cam->height;
    if (prev) launch_gbuffer_motion(s->dev, c, n, alb, nrm, pos, s->upd->d_wv_prev.get(), prev, st); // (rt_gbuffer_motion.hip)
    else hipLaunchKernelGGL(k_gbuffer, dim3((n + 255u) / 256u), dim3(256), 0, st, s->dev, c, alb, nrm, pos);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev, st));
    return RT_OK;
}

// the host variants: the planes on the device, then copied out; `out` has three planes, or four with the motion guide (PRE: the checks passed)
int gbuffer_to_host(rt_scene* s, const rt_camera* cam, std::initializer_list<float*> out) {
    HIPCHK(hipSetDevice(s->device));
    const size_t n = (size_t)cam->width * (size_t)cam->height;
    DevBuf b;
    HIPCHK(b.alloc(out.size() * n * 16u));
    float4* d = b.as<float4>();
    if (const int rc = gbuffer_enqueue(s, cam, d, d + n, d + 2 * n, out.size() == 4 ? d + 3 * n : nullptr, 0)) return rc;
    HIPCHK(hipStreamSynchronize(0));
    const float4* src = d;
    for (float* plane : out) {
        HIPCHK(hipMemcpy(plane, src, n * 16u, hipMemcpyDeviceToHost));
        src += n;
    }
    return RT_OK;
}

} // namespace

extern "C" {

int rt_scene_gbuffer(rt_scene* s, const rt_camera* cam, float* albedo, float* normal, float* position) {
    if (!albedo || !normal || !position) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = gbuffer_check(s, cam)) return rc;
    return gbuffer_to_host(s, cam, {albedo, normal, position});
}

int rt_scene_gbuffer_device(rt_scene* s, const rt_camera* cam, void* d_albedo, void* d_normal, void* d_position, void* stream) {
    if (!d_albedo || !d_normal || !d_position) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = gbuffer_check(s, cam)) return rc;
    return gbuffer_enqueue(s, cam, (float4*)d_albedo, (float4*)d_normal, (float4*)d_position, nullptr, (hipStream_t)stream);
}

int rt_scene_gbuffer_motion(rt_scene* s, const rt_camera* cam, float* albedo, float* normal, float* position, float* prev_position) {
    if (!albedo || !normal || !position || !prev_position) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = gbuffer_check(s, cam)) return rc;
    if (const int rc = motion_check(s)) return rc;
    return gbuffer_to_host(s, cam, {albedo, normal, position, prev_position});
}

int rt_scene_gbuffer_motion_device(rt_scene* s, const rt_camera* cam, void* d_albedo, void* d_normal, void* d_position, void* d_prev_position,
                                   void* stream) {
    if (!d_albedo || !d_normal || !d_position || !d_prev_position) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = gbuffer_check(s, cam)) return rc;
    if (const int rc = motion_check(s)) return rc;
    return gbuffer_enqueue(s, cam, (float4*)d_albedo, (float4*)d_normal, (float4*)d_position, (float4*)d_prev_position, (hipStream_t)stream);
}

} // extern "C"

