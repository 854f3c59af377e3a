// rt_abi.hip — the C entry points of include/rt_mi355x.h for scenes, renderers and frames: argument checks and object life time. What a frame
// launches is rt_frame.hip; the gather rt_comm.hip; the probes rt_probes.hip.
#include "bvh_quantise.h"
#include "rt_internal.h"
#include "rt_scene_image.h"

namespace rtlib {
thread_local std::string g_err;

// a frame or continuation rendered into the renderer's own tile buffers: the host outputs asked for
int copy_out(const rt_renderer* r, int rc, float* rgba_f32, uint8_t* rgba_u8) {
    if (rc != RT_OK) return rc;
    if (rgba_f32 && r->n_local) HIPCHK(hipMemcpy(rgba_f32, r->d_f32, (size_t)r->n_local * 16, hipMemcpyDeviceToHost));
    if (rgba_u8 && r->n_local) HIPCHK(hipMemcpy(rgba_u8, r->d_u8, (size_t)r->n_local * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}
} // namespace rtlib

extern "C" {

const char* rt_last_error(void) { return g_err.c_str(); }
int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(RT_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return n;
}

// Camera::Camera (src/camera.hpp:74-106). Host arithmetic, same operation order as the reference's
// constructor: normalize, two cross products, viewport (aspect, 1), pixel00, per-pixel deltas.
int rt_camera_init(rt_camera* out, int32_t width, int32_t height, const float center[3], const float dir_in[3],
                   float focal_length) {
    if (!out || !center || !dir_in || width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "bad camera arguments");
    auto norm = [](const float v[3], float o[3]) {
        float inv = 1.0f / std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        o[0] = v[0] * inv, o[1] = v[1] * inv, o[2] = v[2] * inv;
    };
    auto cross = [](const float a[3], const float b[3], float o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
    };
    float dir[3], right[3], up[3], tmp[3];
    const float world_up[3] = {0.0f, 1.0f, 0.0f};
    norm(dir_in, dir);
    cross(dir, world_up, tmp), norm(tmp, right);
    cross(right, dir, tmp), norm(tmp, up);
    const float vp0 = 1.0f * ((float)width / (float)height), vp1 = 1.0f;
    const float du_div = (float)width / (vp0 * 2.0f), dv_div = (float)height / (vp1 * 2.0f);
    for (int a = 0; a < 3; ++a) {
        const float viewport_u = (-right[a]) * vp0, viewport_v = up[a] * vp1;
        out->center[a] = center[a];
        out->pixel00[a] = ((center[a] + viewport_u) + viewport_v) + dir[a] * focal_length;
        out->delta_u[a] = right[a] / du_div;
        out->delta_v[a] = (-up[a]) / dv_div;
    }
    out->width = width, out->height = height;
    return RT_OK;
}

int rt_scene_create(const rt_scene_desc* desc, int device, int bvh_kind, rt_scene** out) { return rt_scene_create_ex(desc, device, bvh_kind, 0u, out); }

int rt_scene_create_ex(const rt_scene_desc* desc, int device, int bvh_kind, uint32_t flags, rt_scene** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (flags & ~(RT_SCENE_UPDATABLE | RT_SCENE_KEEP_PREVIOUS)) return fail(RT_ERR_INVALID, "unknown scene flags");
    if ((flags & RT_SCENE_KEEP_PREVIOUS) && !(flags & RT_SCENE_UPDATABLE)) return fail(RT_ERR_INVALID, "RT_SCENE_KEEP_PREVIOUS is a flag of updatable scenes: pass RT_SCENE_UPDATABLE with it");
    if (bvh_kind != RT_BVH_DEFAULT && bvh_kind != RT_BVH_LBVH && bvh_kind != RT_BVH_SAH && bvh_kind != RT_BVH_LBVH_GPU)
        return fail(RT_ERR_INVALID, "unknown bvh_kind");
    if (bvh_kind == RT_BVH_LBVH_GPU) { // the build itself runs on the device
        if (device < 0) return fail(RT_ERR_NO_DEVICE, "RT_BVH_LBVH_GPU needs a device (device >= 0)");
        int rc0 = device_ok(device);
        if (rc0 != RT_OK) return rc0;
    }
    std::unique_ptr<rt_scene, decltype(&rt_scene_destroy)> s(new (std::nothrow) rt_scene(), &rt_scene_destroy); // (every early return frees what the scene holds by then)
    if (!s) return fail(RT_ERR_OOM, "host allocation failed");
    std::string err;
    int rc = RT_OK;
    try {
        rc = build_host_scene(desc, bvh_kind, s->hs, err);
    } catch (const std::bad_alloc&) {
        return fail(RT_ERR_OOM, "host allocation failed while building the scene");
    } catch (const std::exception& e) { // nothing may cross the C ABI as an exception
        return fail(RT_ERR_INVALID, std::string("scene build failed: ") + e.what());
    }
    if (rc != RT_OK) return fail(rc, err);
    const bool updatable = (flags & RT_SCENE_UPDATABLE) != 0;
    // the origin skip (rt_types.h: SkipRec): static host-built trees only — vertices that move break coplanarity, and a device-built tree has no host pass
    rc = no_throw([&] {
        if (updatable || s->hs.built_by == RT_BVH_LBVH_GPU) clear_skip_table(s->hs);
        else build_skip_table(s->hs);
        return (int)RT_OK;
    });
    if (rc != RT_OK) return rc;
    s->device = device;
    if (device >= 0) {
        if ((rc = device_ok(device)) != RT_OK) return rc;
        if (const char* e = dev_knob("RT_INJECT_ALLOC_FAILURE")) s->alloc.inject = std::atoi(e);
        rc = no_throw([&]() -> int { // the device image (rt_scene_image.h)
            const HostScene& hs = s->hs;
            if (hs.nodes.size() > kMaxDeviceNodes) return fail(RT_ERR_INVALID, "BVH too large for 32-bit node offsets");
            SceneAlloc& al = s->alloc;
            uint64_t& bytes = s->device_bytes;
            if (const int e = s->d_nodes.upload(al, device_nodes(hs.nodes), bytes)) return e;
            if (const int e = s->d_tris.upload(al, pack_tris(hs.tris), bytes)) return e;
            if (const int e = s->d_shade.upload(al, hs.shade, bytes)) return e;
            if (const int e = s->d_skip.upload(al, hs.skip, bytes)) return e;
            std::vector<InstRec> rows(hs.inst); // (an updatable scene's table has room for a row per instance: the distinct matrices may grow)
            if (updatable) rows.resize(std::max<size_t>(rows.size(), desc->n_instances));
            if (const int e = s->d_inst.upload(al, rows, bytes)) return e;
            if (const int e = s->d_mats.upload(al, hs.mats, bytes)) return e;
            if (const int e = s->d_tex.upload(al, hs.tex, bytes)) return e;
            uint64_t uncounted = 0; // (the query cursors, rt_query_launch.h, are no part of device_bytes)
            if (s->d_query_cursor.upload(al, nullptr, kQueryCursorBytes / 8u, uncounted) != RT_OK)
                return fail(RT_ERR_OOM, "device allocation failed (the ray-query cursors)");
            s->dev.nodes = s->d_nodes.get(), s->dev.tris = s->d_tris.get(), s->dev.shade = s->d_shade.get(), s->dev.skip = s->d_skip.get();
            s->dev.inst = s->d_inst.get(), s->dev.mats = s->d_mats.get(), s->dev.tex = s->d_tex.get();
            scene_scalars(hs, s->dev);
            return RT_OK;
        });
        if (rc != RT_OK) return rc;
    }
    if (updatable && (rc = no_throw([&] { return init_scene_update(s.get(), desc, (flags & RT_SCENE_KEEP_PREVIOUS) != 0); })) != RT_OK) return rc;
    *out = s.release();
    return RT_OK;
}

// the scene's device current, every reader's last launch done (rt_scene::readers); the members then free what they own
void rt_scene_destroy(rt_scene* s) {
    if (!s) return;
    if (s->device >= 0 && hipSetDevice(s->device) == hipSuccess)
        for (auto& se : s->readers) (void)hipEventSynchronize(se.second), (void)hipEventDestroy(se.second);
    delete s;
}

int rt_scene_info(const rt_scene* s, rt_scene_info_t* out) {
    if (!s || !out) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = sync_host_copy(s)) return rc;
    out->n_triangles = (uint32_t)(s->hs.wverts.size() / 9);
    out->n_nodes = (uint32_t)s->hs.nodes.size();
    out->max_depth = s->hs.max_depth;
    out->max_leaf_tris = s->hs.max_leaf_tris;
    std::memcpy(out->bounds_lo, s->hs.bounds_lo, 12), std::memcpy(out->bounds_hi, s->hs.bounds_hi, 12);
    out->sah_cost = s->hs.sah_cost;
    out->device_bytes = s->device_bytes;
    out->n_leaf_records = (uint32_t)s->hs.tris.size();
    out->n_split_triangles = s->hs.n_split_triangles;
    return RT_OK;
}

int rt_scene_check_bvh(const rt_scene* s) {
    if (!s) return fail(RT_ERR_INVALID, "null scene");
    if (const int rc0 = sync_host_copy(s)) return rc0;
    std::string err;
    int rc = check_bvh(s->hs, err);
    return rc == RT_OK ? RT_OK : fail(rc, err);
}

int rt_scene_count_visits(const rt_scene* s, uint32_t n, const float* org, const float* dir, int mode, uint64_t* node_visits, uint64_t* tri_tests,
                          float* t, uint32_t* tri) {
    if (!s || (n && (!org || !dir))) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc0 = sync_host_copy(s)) return rc0;
    std::string err;
    const int rc = no_throw([&] { return count_visits(s->hs, n, org, dir, mode, node_visits, tri_tests, t, tri, err); });
    return rc == RT_OK ? RT_OK : fail(rc, err.empty() ? g_err : err);
}

int rt_renderer_create(int kind, rt_scene* scene, int32_t width, int32_t height, uint32_t max_depth,
                       uint32_t sample_count, uint32_t seed_mode, rt_renderer** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (!scene) return fail(RT_ERR_INVALID, "null scene");
    if (kind != RT_RENDERER_MEGAKERNEL && kind != RT_RENDERER_WAVEFRONT) return fail(RT_ERR_INVALID, "unknown renderer kind");
    if (width <= 0 || height <= 0 || (int64_t)width * height > (int64_t)1 << 30) return fail(RT_ERR_INVALID, "bad image size");
    if (sample_count == 0) return fail(RT_ERR_INVALID, "sample_count must be >= 1");
    if (seed_mode > RT_SEED_MEGAKERNEL) return fail(RT_ERR_INVALID, "unknown seed mode");
    if ((uint64_t)sample_count * ((uint64_t)max_depth + 1) > (1ull << 26)) return fail(RT_ERR_INVALID, "sample_count * max_depth too large");
    if (scene->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    int rc = device_ok(scene->device);
    if (rc != RT_OK) return rc;
    rt_renderer* r = new (std::nothrow) rt_renderer();
    if (!r) return fail(RT_ERR_OOM, "host allocation failed");
    r->kind = kind, r->scene = scene, r->width = width, r->height = height;
    r->scene_gen = scene->generation;
    r->max_depth = max_depth, r->spp = sample_count;
    r->seed_mode = seed_mode != RT_SEED_DEFAULT ? seed_mode
                   : (kind == RT_RENDERER_MEGAKERNEL ? RT_SEED_MEGAKERNEL : RT_SEED_WAVEFRONT);
    r->hw_queues = hw_queues_from_env();
    const char* prof = std::getenv("RT_PROFILE_KERNELS");
    r->profile_kernels = prof && prof[0] == '1';
    if (const char* e = dev_knob("RT_MEGA_LDS_PAD")) r->mega_lds_pad = (uint32_t)std::max(0, std::min(100 * 1024, std::atoi(e)));
    if (const char* e = dev_knob("RT_MEGA_OCC")) r->mega_occ = (uint32_t)std::max(1, std::min((int)kMegaWaves, std::atoi(e)));
    auto bail = [&](int code) {
        rt_renderer_destroy(r);
        return code;
    };
    { // the device's lane-stream pool is set up by the FIRST renderer of either kind (see lane_stream_of: early, and in one burst)
        hipStream_t s0 = nullptr;
        bool owned = false;
        if (lane_stream_of(scene->device, 0, &s0, &owned) != hipSuccess) return bail(fail(RT_ERR_HIP, "cannot create the stream-lane pool"));
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, scene->device) == hipSuccess && prop.multiProcessorCount > 0) r->n_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(RT_ERR_HIP, "hipStreamCreate failed"));
    if (hipEventCreate(&r->ev_begin) != hipSuccess || hipEventCreate(&r->ev_end) != hipSuccess ||
        hipEventCreateWithFlags(&r->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&r->ev_tile_read, hipEventDisableTiming) != hipSuccess)
        return bail(fail(RT_ERR_HIP, "hipEventCreate failed"));
    // (the megakernel's camera and slices; the wavefront renderer's one-launch schedule uses the slices part)
    if (hipMalloc((void**)&r->d_frame, sizeof(MegaFrame)) != hipSuccess || hipHostMalloc((void**)&r->h_frame, sizeof(MegaFrame)) != hipSuccess)
        return bail(fail(RT_ERR_OOM, "frame constant buffer allocation failed"));
    if (kind == RT_RENDERER_WAVEFRONT) {
        if (hipMalloc((void**)&r->d_cam, sizeof(CameraDev)) != hipSuccess || hipHostMalloc((void**)&r->h_cam, sizeof(CameraDev)) != hipSuccess)
            return bail(fail(RT_ERR_OOM, "camera buffer allocation failed"));
        // Environment shim for sweep scripts, DEVELOPER builds only (rt_knobs.h; the API is rt_renderer_set_schedule): the variables fill the initial schedule.
        // RT_WF_STREAMS / RT_WF_REQUEUE alone have always meant "not the one-launch schedule": they imply a launch per sample.
        rt_schedule& sc = r->sched;
        if (const char* e = dev_knob("RT_WF_GRAPH")) sc.hip_graph = e[0] == '1';
        if (const char* e = dev_knob("RT_WF_FINISH_DEPTH")) sc.finish_depth = (uint32_t)std::max(0, std::atoi(e));
        if (const char* e = dev_knob("RT_WF_SAMPLES_PER_LAUNCH")) sc.samples_per_launch = (uint32_t)std::max(0, std::atoi(e));
        if (const char* e = dev_knob("RT_WF_REQUEUE")) sc.requeue = e[0] != '0' ? 1 : 0;
        if (const char* e = dev_knob("RT_WF_STREAMS")) sc.stream_lanes = (uint32_t)std::max(1, std::min(8, std::atoi(e)));
        if ((dev_knob("RT_WF_REQUEUE") || dev_knob("RT_WF_STREAMS")) && sc.samples_per_launch == 0) sc.samples_per_launch = 1;
        if (const char* e = dev_knob("RT_WF_LPT")) sc.cost_order = e[0] == '0' ? 0 : (e[0] == '2' ? 1 : -1); // 2: forced
        if (const char* e = dev_knob("RT_WF_EXTEND_OCC")) r->wf_extend_occ = (uint32_t)std::max(1, std::min((int)kExtendWaves, std::atoi(e)));
        if (const char* e = dev_knob("RT_WF_FINISH_OCC")) r->wf_finish_occ = (uint32_t)std::max(1, std::min((int)kMegaWaves, std::atoi(e)));
        if (const char* e = dev_knob("RT_WF_SHOOT_CHUNK")) r->wf_shoot_chunk = (uint32_t)std::max(16, std::min(1024, std::atoi(e)));
        if (const char* e = dev_knob("RT_WF_SHOOT_TAIL")) r->wf_shoot_tail = e[0] == '1';
        if (const char* e = dev_knob("RT_WF_SHOOT_STATIC_PCT")) r->wf_shoot_static_pct = (uint32_t)std::max(0, std::min(100, std::atoi(e)));
        if (const char* e = dev_knob("RT_WF_REORDER")) sc.reorder = e[0] == '1';
        if (const char* e = dev_knob("RT_WF_MATSORT")) sc.matsort = e[0] == '1';
        if (const char* e = dev_knob("RT_WF_FUSED_BOUNCE")) sc.fused_bounce = e[0] == '1';
    }
    rc = no_throw([&] { return alloc_tile_buffers(r); });
    if (rc != RT_OK) return bail(rc);
    *out = r;
    return RT_OK;
}

void rt_renderer_destroy(rt_renderer* r) {
    if (!r) return;
    if (r->scene && r->frame_pending && r->scene->frames_pending) r->scene->frames_pending--;
    if (r->scene && hipSetDevice(r->scene->device) == hipSuccess) {
        drain_streams(r, r->pending.stream);
        free_tile_buffers(r);
        if (r->d_cam) (void)hipFree(r->d_cam);
        if (r->h_cam) (void)hipHostFree(r->h_cam);
        if (r->d_frame) (void)hipFree(r->d_frame);
        if (r->h_frame) (void)hipHostFree(r->h_frame);
        for (hipEvent_t e : r->ev_pool) (void)hipEventDestroy(e);
        if (r->ev_begin) (void)hipEventDestroy(r->ev_begin);
        if (r->ev_end) (void)hipEventDestroy(r->ev_end);
        if (r->ev_fork) (void)hipEventDestroy(r->ev_fork);
        if (r->ev_tile_read) (void)hipEventDestroy(r->ev_tile_read);
        if (r->stream) (void)hipStreamDestroy(r->stream);
    }
    delete r;
}

int rt_renderer_set_tile(rt_renderer* r, uint32_t rank, uint32_t world, uint32_t strip_rows) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    if (world == 0 || rank >= world || strip_rows == 0) return fail(RT_ERR_INVALID, "bad tile split");
    if (r->frame_pending) return fail(RT_ERR_INVALID, "a frame is in flight (rt_render_frame_end first)");
    HIPCHK(hipSetDevice(r->scene->device));
    drain_streams(r, r->pending.stream); // the queues are about to be freed: nothing may be running on any of the renderer's streams
    const TileDev old = r->tile;
    r->tile.rank = rank, r->tile.world = world, r->tile.strip_rows = strip_rows;
    const int rc = no_throw([&] { return alloc_tile_buffers(r); });
    if (rc != RT_OK) r->tile.rank = old.rank, r->tile.world = old.world, r->tile.strip_rows = old.strip_rows;
    return rc;
}

int32_t rt_renderer_local_rows(const rt_renderer* r) { return r ? r->tile.local_rows : 0; }

int32_t rt_renderer_global_row(const rt_renderer* r, int32_t local_row) {
    if (!r || local_row < 0 || local_row >= r->tile.local_rows) return -1;
    const uint32_t strip = (uint32_t)local_row / r->tile.strip_rows, within = (uint32_t)local_row % r->tile.strip_rows;
    return (int32_t)((strip * r->tile.world + r->tile.rank) * r->tile.strip_rows + within);
}

int rt_renderer_set_profiling(rt_renderer* r, int enable) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    r->profile_kernels = enable != 0;
    return RT_OK;
}

int rt_renderer_set_russian_roulette(rt_renderer* r, uint32_t start_bounce) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    if (r->rr_start != start_bounce) drop_graph(r); // the bounce flags are baked into the captured launches
    r->rr_start = start_bounce;
    r->carry_samples = 0; // (progressive rendering: the carried chains were rendered with the old paths' ends)
    return RT_OK;
}

int rt_renderer_set_frame_seed(rt_renderer* r, uint32_t salt) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    if (r->frame_pending) return fail(RT_ERR_INVALID, "a frame is in flight (rt_render_frame_end first)");
    if (r->frame_salt != salt) drop_graph(r); // k_wf_init's seed offset is baked into the captured launches
    r->frame_salt = salt; // (a continuation goes on from the carried RNG words: the chain keeps the salt it was started with)
    return RT_OK;
}

int rt_renderer_get_schedule(const rt_renderer* r, rt_schedule* out) {
    if (!r || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = r->sched;
    return RT_OK;
}

int rt_renderer_set_schedule(rt_renderer* r, const rt_schedule* s) {
    if (!r || !s) return fail(RT_ERR_INVALID, "null argument");
    if (s->stream_lanes > 8) return fail(RT_ERR_INVALID, "at most 8 stream lanes");
    if (s->requeue < -1 || s->requeue > 1 || s->cost_order < -1 || s->cost_order > 1 || s->reorder > 1 || s->matsort > 1 || s->hip_graph > 1 || s->fused_bounce > 1)
        return fail(RT_ERR_INVALID, "schedule field out of range");
    if (r->frame_pending) return fail(RT_ERR_INVALID, "a frame is in flight (rt_render_frame_end first)");
    if (s->pixel_slices < -1 || s->pixel_slices > (int32_t)kMaxSlices) return fail(RT_ERR_INVALID, "pixel_slices: -1 (automatic), 0 or 1 (off), 2 .. 8");
    if (r->kind != RT_RENDERER_WAVEFRONT && wants_slices(s->pixel_slices) == wants_slices(r->sched.pixel_slices)) { // the megakernel is one launch: only its pixel slices are a choice (their state buffer exists or not)
        r->sched = *s;
        r->carry_samples = 0; // (progressive rendering: a new schedule discards the carried state)
        return RT_OK;
    }
    HIPCHK(hipSetDevice(r->scene->device));
    drain_streams(r, r->pending.stream); // the queues are re-allocated (stream lanes, second queue, hit records, dynamic queue)
    const rt_schedule old = r->sched;
    r->sched = *s;
    const int rc = no_throw([&] { return alloc_tile_buffers(r); });
    if (rc != RT_OK) r->sched = old; // the buffers are gone (frames are refused), the schedule on record is the last one that worked
    return rc;
}

int rt_render_frame(rt_renderer* r, const rt_camera* cam, float* rgba_f32, uint8_t* rgba_u8, rt_stats* stats) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return copy_out(r, no_throw([&] { return render_impl(r, cam, rgba_f32 ? r->d_f32 : nullptr, rgba_u8 ? r->d_u8 : nullptr, r->stream, stats); }), rgba_f32, rgba_u8);
}

int rt_render_frame_device(rt_renderer* r, const rt_camera* cam, void* d_rgba_f32, void* d_rgba_u8, void* stream,
                           rt_stats* stats) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return no_throw([&] { return render_impl(r, cam, (float*)d_rgba_f32, (uint8_t*)d_rgba_u8, stream ? (hipStream_t)stream : r->stream, stats); });
}

int rt_renderer_set_progressive(rt_renderer* r, int enable) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    if (r->frame_pending) return fail(RT_ERR_INVALID, "a frame is in flight (rt_render_frame_end first)");
    HIPCHK(hipSetDevice(r->scene->device));
    drop_graph(r); // (a captured frame stores the carried state or does not)
    r->progressive = enable != 0;
    const int rc = no_throw([&] { return alloc_carry(r); });
    if (rc != RT_OK) r->progressive = false;
    return rc;
}

int rt_render_frame_continue(rt_renderer* r, uint32_t samples, float* rgba_f32, uint8_t* rgba_u8, rt_stats* stats) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return copy_out(r, no_throw([&] { return continue_impl(r, samples, rgba_f32 ? r->d_f32 : nullptr, rgba_u8 ? r->d_u8 : nullptr, r->stream, stats); }), rgba_f32, rgba_u8);
}

int rt_render_frame_continue_device(rt_renderer* r, uint32_t samples, void* d_rgba_f32, void* d_rgba_u8, void* stream, rt_stats* stats) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return no_throw([&] { return continue_impl(r, samples, (float*)d_rgba_f32, (uint8_t*)d_rgba_u8, stream ? (hipStream_t)stream : r->stream, stats); });
}

int rt_renderer_accumulated_samples(const rt_renderer* r, uint32_t* out) {
    if (!r || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = carry_is_current(r) ? r->carry_samples : 0u; // (a scene update ends the chain)
    return RT_OK;
}

int rt_renderer_block_grid(const rt_renderer* r, uint32_t* blocks_x, uint32_t* blocks_y) {
    if (!r || !blocks_x || !blocks_y) return fail(RT_ERR_INVALID, "null argument");
    *blocks_x = ((uint32_t)r->width + 7u) / 8u, *blocks_y = ((uint32_t)r->tile.local_rows + 7u) / 8u;
    return RT_OK;
}

int rt_renderer_block_samples(const rt_renderer* r, uint32_t* out) {
    if (!r || !out) return fail(RT_ERR_INVALID, "null argument");
    const size_t nb = (size_t)(((uint32_t)r->width + 7u) / 8u) * (((uint32_t)r->tile.local_rows + 7u) / 8u);
    if (r->carry_samples == 0 || !carry_is_current(r) || r->h_block_count.size() != nb) std::memset(out, 0, nb * 4); // nothing to continue
    else std::memcpy(out, r->h_block_count.data(), nb * 4);
    return RT_OK;
}

int rt_renderer_block_errors(const rt_renderer* r, float* out) {
    if (!r || !out) return fail(RT_ERR_INVALID, "null argument");
    return no_throw([&] { return block_errors(r, out); });
}

int rt_render_frame_continue_blocks(rt_renderer* r, uint32_t samples, const uint32_t* blocks, uint32_t n_blocks, float* rgba_f32, uint8_t* rgba_u8,
                                    rt_stats* stats) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return copy_out(r, no_throw([&] { return continue_blocks_impl(r, samples, blocks, n_blocks, rgba_f32 ? r->d_f32 : nullptr, rgba_u8 ? r->d_u8 : nullptr, r->stream, stats); }), rgba_f32, rgba_u8);
}

int rt_render_frame_continue_blocks_device(rt_renderer* r, uint32_t samples, const uint32_t* blocks, uint32_t n_blocks, void* d_rgba_f32, void* d_rgba_u8,
                                           void* stream, rt_stats* stats) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return no_throw([&] {
        return continue_blocks_impl(r, samples, blocks, n_blocks, (float*)d_rgba_f32, (uint8_t*)d_rgba_u8, stream ? (hipStream_t)stream : r->stream, stats);
    });
}

int rt_renderer_adapt(rt_renderer* r, float threshold, uint32_t min_samples, uint32_t* blocks_out, uint32_t* n_out) {
    if (!r || !n_out) return fail(RT_ERR_INVALID, "null argument");
    return no_throw([&]() -> int {
        std::vector<uint32_t> blocks;
        const int rc = adapt_impl(r, threshold, min_samples, blocks);
        if (rc != RT_OK) return rc;
        if (!blocks.empty() && !blocks_out) return fail(RT_ERR_INVALID, "null block list");
        if (!blocks.empty()) std::memcpy(blocks_out, blocks.data(), blocks.size() * 4);
        *n_out = (uint32_t)blocks.size();
        return (int)RT_OK;
    });
}

int rt_render_frame_continue_adaptive(rt_renderer* r, uint32_t samples, float threshold, uint32_t min_samples, float* rgba_f32, uint8_t* rgba_u8,
                                      rt_stats* stats, uint32_t* n_blocks_out) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return copy_out(r, no_throw([&] {
        return continue_adaptive_impl(r, samples, threshold, min_samples, rgba_f32 ? r->d_f32 : nullptr, rgba_u8 ? r->d_u8 : nullptr, r->stream, stats,
                                      n_blocks_out);
    }), rgba_f32, rgba_u8);
}

int rt_render_frame_continue_adaptive_device(rt_renderer* r, uint32_t samples, float threshold, uint32_t min_samples, void* d_rgba_f32, void* d_rgba_u8,
                                             void* stream, rt_stats* stats, uint32_t* n_blocks_out) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return no_throw([&] {
        return continue_adaptive_impl(r, samples, threshold, min_samples, (float*)d_rgba_f32, (uint8_t*)d_rgba_u8, stream ? (hipStream_t)stream : r->stream,
                                      stats, n_blocks_out);
    });
}

int rt_render_frame_begin(rt_renderer* r, const rt_camera* cam, void* d_rgba_f32, void* d_rgba_u8, void* stream) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return no_throw([&] { return frame_begin(r, cam, (float*)d_rgba_f32, (uint8_t*)d_rgba_u8, stream ? (hipStream_t)stream : r->stream); });
}

int rt_render_frame_end(rt_renderer* r, rt_stats* stats) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    return no_throw([&] { return frame_end(r, stats); });
}

} // extern "C"

#ifdef RT_DEVELOPER_KNOBS
// Developer library only: how a scene's shading tables came out (the packed shading word, the distinct-matrix table, what the shading
// kernels stage in LDS), for the tests that must show which path of shade_hit (rt_device.h) a scene takes.
extern "C" {

// packed_mat: ShadeRec::instance carries the material (rt_types.h); lds_nm / lds_mats: entries staged in LDS (0 for a host-only scene:
// only device scenes stage); n_rows: rows of the device's instance table — distinct normal matrices when packed, else one per instance.
// rows: 9 floats per row, the first `capacity` rows (may be null); words: ShadeRec::instance of every triangle in rt_scene_desc order
// (n_triangles entries, may be null).
int rt_dev_scene_tables(const rt_scene* s, uint32_t* packed_mat, uint32_t* lds_nm, uint32_t* lds_mats, uint32_t* n_rows, float* rows,
                        uint32_t capacity, uint32_t* words) {
    if (!s || !packed_mat || !lds_nm || !lds_mats || !n_rows) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = sync_host_copy(s)) return rc;
    *packed_mat = s->hs.packed_mat ? 1u : 0u;
    *lds_nm = s->dev.lds_nm, *lds_mats = s->dev.lds_mats;
    *n_rows = (uint32_t)s->hs.inst.size();
    if (rows)
        for (size_t k = 0; k < std::min<size_t>(capacity, s->hs.inst.size()); ++k) std::memcpy(rows + 9 * k, s->hs.inst[k].normal_mat, 36);
    if (words)
        for (size_t t = 0; t < s->hs.shade.size(); ++t) words[t] = s->hs.shade[t].instance;
    return RT_OK;
}

// The scene's BVH as built, for the tests that hold the device-built tree against a model of it (tests/test_gpu_lbvh.py). Scalars:
// n_nodes, n_tris (leaf-order records), n_wverts (floats), stack_need, built_by (RT_BVH_LBVH_GPU: built on the device; 99 =
// RT_BVH_MEDIAN_INTERNAL: the balanced host fallback; else the host builder asked for); pad and bounds[6] (lo xyz, hi xyz) as the builder
// used them. Arrays (each may be null, else takes the first `capacity` entries): nodes as raw 64-byte BvhNode records (the host copy: child
// words are node indices), every leaf record's global_index, and the fp32 world-space vertices (9 per triangle, scene order).
int rt_dev_scene_tree(const rt_scene* s, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* n_wverts, uint32_t* stack_need, int32_t* built_by,
                      float* pad, float* bounds, void* nodes, uint32_t* global_index, float* wverts, uint32_t capacity) {
    if (!s || !n_nodes || !n_tris || !n_wverts || !stack_need || !built_by || !pad || !bounds) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = sync_host_copy(s)) return rc;
    const HostScene& hs = s->hs;
    *n_nodes = (uint32_t)hs.nodes.size(), *n_tris = (uint32_t)hs.tris.size(), *n_wverts = (uint32_t)hs.wverts.size();
    *stack_need = hs.stack_need, *built_by = hs.built_by, *pad = hs.pad;
    for (int a = 0; a < 3; ++a) bounds[a] = hs.bounds_lo[a], bounds[3 + a] = hs.bounds_hi[a];
    if (nodes) std::memcpy(nodes, hs.nodes.data(), std::min<size_t>(capacity, hs.nodes.size()) * sizeof(BvhNode));
    if (global_index)
        for (size_t t = 0; t < std::min<size_t>(capacity, hs.tris.size()); ++t) global_index[t] = hs.tris[t].global_index;
    if (wverts) std::memcpy(wverts, hs.wverts.data(), std::min<size_t>(capacity, hs.wverts.size()) * sizeof(float));
    return RT_OK;
}

// The origin-skip table of the scene's HOST copy (rt_types.h: SkipRec, 8 words per triangle): write = 0 copies the first `capacity` entries
// out, write = 1 overwrites them from `entries` — what rt_scene_check_bvh then examines (the device's copy is not touched).
int rt_dev_scene_skip_table(rt_scene* s, uint32_t* n_entries, uint32_t* entries, uint32_t capacity, int write) {
    if (!s || !n_entries) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = sync_host_copy(s)) return rc;
    *n_entries = (uint32_t)s->hs.skip.size();
    const size_t n = std::min<size_t>(capacity, s->hs.skip.size());
    if (entries && n) {
        if (write) std::memcpy(s->hs.skip.data(), entries, n * sizeof(SkipRec));
        else std::memcpy(entries, s->hs.skip.data(), n * sizeof(SkipRec));
    }
    return RT_OK;
}

// How many hipGraphs the renderer has captured (rt_schedule::hip_graph = 1): a scene update makes the next frame capture again.
int rt_dev_renderer_graph_captures(const rt_renderer* r, uint32_t* out) {
    if (!r || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = r->graph_captures;
    return RT_OK;
}

// Host only: the quantiser (bvh_quantise.h: quantise_node) as the host runs it, on `count` nodes. nk[i] in 1..4 children; klo/khi: 4 x 3
// floats per node, the children's already padded boxes (entries past nk[i] are ignored; pad = 0 here, and x - 0 and x + 0 keep every x the
// quantiser stores, -0 included); nodes_out: count 64-byte BvhNode records (origin, scales and planes; child words kChildEmpty); ok[i] = 0
// where quantise_node refused the node (a non-finite box or no grid step that fits).
int rt_dev_quantise_node(uint32_t count, const int32_t* nk, const float* klo, const float* khi, void* nodes_out, uint8_t* ok) {
    if (!nk || !klo || !khi || !nodes_out || !ok) return fail(RT_ERR_INVALID, "null argument");
    BvhNode* out = static_cast<BvhNode*>(nodes_out);
    for (uint32_t i = 0; i < count; ++i) {
        if (nk[i] < 1 || nk[i] > 4) return fail(RT_ERR_INVALID, "nk must be 1..4");
        Box3 kb[4];
        for (int k = 0; k < 4; ++k) std::memcpy(kb[k].lo, klo + 12 * (size_t)i + 3 * k, 12), std::memcpy(kb[k].hi, khi + 12 * (size_t)i + 3 * k, 12);
        out[i] = empty_node();
        ok[i] = quantise_node(out[i], nk[i], kb, 0.0f) ? 1 : 0;
    }
    return RT_OK;
}

} // extern "C"
#endif
