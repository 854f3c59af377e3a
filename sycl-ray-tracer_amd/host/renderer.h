// renderer.h — C++ host mirror of the reference's renderer plugin surface, over the C ABI of
// librt_mi355x.so. Same names and argument meaning as the reference; SYCL/Embree types are replaced by
// plain ones. Errors of the C ABI become std::runtime_error (main() turns them into a message + non-zero
// exit, where the reference calls std::terminate: src/main.cpp:71-74).
//
//   raytracer::Camera               == src/camera.hpp:65-106
//   raytracer::Scene                == src/scene.hpp:64-100 (loader in scene_loader.cpp)
//   raytracer::IRenderer            == src/render.hpp:11-18
//   raytracer::MegakernelRenderer   == src/render_megakernel.hpp:10-22, render_frame src/render_megakernel.cpp:75-187
//   raytracer::WavefrontRenderer    == src/render_wavefront.hpp:40-76,  render_frame src/render_wavefront.cpp:396-431
#pragma once
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/rt_mi355x.h"
#include "png.h"
#include "scene_loader.h"

namespace raytracer {

inline void rt_check(int status) {
    if (status != RT_OK) throw std::runtime_error(std::string("librt_mi355x: ") + rt_last_error());
}

struct Camera {
    rt_camera c{};
    // Camera(img_size, cam_center, cam_dir, focal_length): src/camera.hpp:74-106
    Camera(std::array<int32_t, 2> img_size, const float center[3], const float dir[3], float focal_length) {
        rt_check(rt_camera_init(&c, img_size[0], img_size[1], center, dir, focal_length));
    }
};

struct Scene {
    rthost::LoadedScene data;
    rt_scene* handle = nullptr;
    int device = 0, bvh_kind = RT_BVH_DEFAULT;
    mutable std::map<int, rt_scene*> replicas; // device -> scene replica (multi-GPU frames), built on first use
    float camera_position[3], camera_direction[3], camera_focal_length;

    // Scene(app, filepath): src/scene.cpp:54-129. `device` replaces App's SYCL device.
    // flags: RT_SCENE_UPDATABLE for a scene that spin() moves between frames
    Scene(const std::string& filepath, int device = 0, int bvh_kind = RT_BVH_DEFAULT, bool verbose = true, uint32_t flags = 0)
        : data(rthost::load_glb(filepath, verbose)), device(device), bvh_kind(bvh_kind) {
        for (int k = 0; k < 3; ++k) camera_position[k] = data.camera_position[k], camera_direction[k] = data.camera_direction[k];
        camera_focal_length = data.camera_focal_length;
        const rt_scene_desc d = data.desc();
        rt_check(rt_scene_create_ex(&d, device, bvh_kind, flags, &handle));
        rt_scene_info_t info{};
        rt_check(rt_scene_info(handle, &info));
        for (int k = 0; k < 3; ++k) spin_centre[k] = 0.5f * (info.bounds_lo[k] + info.bounds_hi[k]);
    }
    float spin_centre[3] = {0, 0, 0}; // the centre of the scene's bounds as loaded

    // Every instance turned by `deg` degrees (from its loaded pose) about the vertical axis through spin_centre: rt_scene_update of an
    // updatable scene. normal_mat = transpose(inverse(mat3(transform))) as the loader makes it.
    rt_update_stats spin(double deg) {
        const double a = deg * 3.14159265358979323846 / 180.0;
        const float c = (float)std::cos(a), s = (float)std::sin(a);
        // R about y through the centre, column-major: x' = c x + s z, z' = -s x + c z (+ the translation that keeps the centre)
        float r[16] = {c, 0, -s, 0, 0, 1, 0, 0, s, 0, c, 0, 0, 0, 0, 1};
        r[12] = spin_centre[0] - (c * spin_centre[0] + s * spin_centre[2]);
        r[14] = spin_centre[2] - (-s * spin_centre[0] + c * spin_centre[2]);
        std::vector<rt_instance> inst(data.instances);
        for (rt_instance& in : inst) {
            float m[16];
            for (int col = 0; col < 4; ++col)
                for (int row = 0; row < 4; ++row) {
                    float v = 0.0f;
                    for (int k = 0; k < 4; ++k) v += r[k * 4 + row] * in.transform[col * 4 + k];
                    m[col * 4 + row] = v;
                }
            std::memcpy(in.transform, m, sizeof(m));
            // cofactors of the 3x3 part: inverse-transpose = cofactor matrix / det
            auto e = [&](int col, int row) { return m[col * 4 + row]; };
            float cof[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
                    cof[i][j] = e(i1, j1) * e(i2, j2) - e(i1, j2) * e(i2, j1); // cofactor of column i, row j
                }
            const float det = e(0, 0) * cof[0][0] + e(0, 1) * cof[0][1] + e(0, 2) * cof[0][2];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) in.normal_mat[i * 3 + j] = cof[i][j] / det;
        }
        rt_scene_update_desc u{};
        u.n_instances = (uint32_t)inst.size();
        u.instances = inst.data();
        rt_update_stats st{};
        rt_check(rt_scene_update(handle, &u, &st));
        return st;
    }
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    ~Scene() {
        for (auto& kv : replicas) rt_scene_destroy(kv.second);
        rt_scene_destroy(handle);
    }
    // the scene on `dev`: the primary handle or a replica (every GPU of a tiled frame holds the whole scene + BVH)
    rt_scene* on_device(int dev) const {
        if (dev == device) return handle;
        auto it = replicas.find(dev);
        if (it != replicas.end()) return it->second;
        const rt_scene_desc d = data.desc();
        rt_scene* h = nullptr;
        rt_check(rt_scene_create(&d, dev, bvh_kind, &h));
        replicas[dev] = h;
        return h;
    }
};

struct IRenderer {
    virtual void render_frame(const Camera& camera, const Scene& scene) = 0;
    virtual ~IRenderer() {}
};

// Shared body of the two renderers: they differ only in the `kind` handed to the C ABI.
struct HipRendererBase : public IRenderer {
    std::array<int32_t, 2> img_size;
    uint8_t* image; // caller-owned RGBA8 buffer, W*H*4 (the reference's malloc_shared image: src/main.cpp:39-46)
    const uint32_t max_depth, sample_count;
    rt_renderer* handle = nullptr;
    const Scene* bound = nullptr;
    int kind;
    std::string out_path = "out.png"; // src/util.hpp:27
    uint32_t russian_roulette = 0;    // extension, 0 = off (rt_renderer_set_russian_roulette)
    // Extension: which of the wavefront renderer's schedules renders the frame (rt_renderer_set_schedule; same frame bit for bit). The
    // reference has one, a launch per bounce (src/render_wavefront.cpp:396-417): finish_depth = RT_SCHED_ALL_BOUNCES. Ignored by the megakernel.
    rt_schedule schedule{0u, 0u, 0u, -1, 0u, 0u, -1, 0u, 0u, -1};
    bool has_schedule = false;
    // Extension: more than one entry tiles the frame over these HIP devices in THIS process, one host thread per
    // tile (interleaved 8-row strips, tile k -> devices[k]; the same device may appear more than once). Every tile is
    // rendered into its renderer's own device buffer; rt_frame_gather then brings the strips to devices[0] with one
    // grouped ncclGather over xGMI and de-interleaves them there: the frame touches host memory once, for the PNG.
    // (The one-process-per-GPU form of the same gather is rtamd/dist.py + bench.py.)
    std::vector<int> devices;
    // Extension: progressive rendering (rt_renderer_set_progressive). passes > 1 renders sample_count samples, then continues the frame
    // passes - 1 times by sample_count samples (rt_render_frame_continue): the image of sample_count x passes samples, bit for bit.
    uint32_t passes = 1;
    // Extension: adaptive sampling. adaptive >= 0: passes 2 .. K continue only the 8x8 blocks rt_renderer_adapt finds active (threshold
    // `adaptive` on the two-image error, blocks under min_samples samples always) — rt_render_frame_continue_adaptive; every rank adapts its own
    float adaptive = -1.0f;
    uint32_t min_samples = 0;
    // Extension: denoise > 0 runs the a-trous denoiser (rt_denoise_device, `denoise` iterations, the defaults of rtamd/renderer.py) on the frame
    // after its last pass, guided by the G-buffer of the camera (rt_scene_gbuffer_device), and writes the denoised unorm8 image. A tiled frame is
    // denoised on the root device after the gather (its fp32 plane gathered too), with the root's scene. Everything stays on that device.
    uint32_t denoise = 0;
    std::vector<float> frame_f32;
    rt_denoiser* denoiser = nullptr;
    float* d_gbuf = nullptr;      // the three guide planes, W*H*4 floats each (on den_device)
    uint8_t* d_den_u8 = nullptr;  // the denoised unorm8 image
    hipStream_t den_stream = nullptr;
    hipEvent_t den_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int den_device = -1;
    // Extension: guided > 0 (with denoise > 0) replaces rt_denoise by the variance-guided filter with sigma_luminance = guided
    // (rt_denoise_variance_device + rt_denoise_guided_device, the other defaults of rtamd/renderer.py). With temporal > 0 the accumulator carries the
    // luminance moments (RT_TEMPORAL_MOMENTS) and the variance comes from them where the history is long enough; without it the estimate is spatial.
    float guided = 0.0f;
    float* d_var = nullptr;       // the variance plane between the estimate and the filter, W*H floats (on den_device)
    float* d_tmp_mom = nullptr;   // the accumulated moments, W*H*2 floats, and
    float* d_tmp_len = nullptr;   // the history lengths, W*H floats (on tmp_device): what the variance estimate reads
    // Extension: temporal > 0 (one device, frames of an animation): every frame is rendered with its own seed salt (frame_salt,
    // rt_renderer_set_frame_seed) and accumulated over the frames before it (rt_scene_gbuffer_motion_device + rt_temporal_accumulate_device,
    // max_history = temporal, the defaults of rtamd/renderer.py) before it is denoised (if asked for) and written. The scene must keep its
    // previous vertices (RT_SCENE_KEEP_PREVIOUS). temporal == 0: salt 0, nothing of this runs.
    uint32_t temporal = 0;
    uint32_t frame_salt = 0;
    rt_temporal* accumulator = nullptr;
    float* d_tmp_gbuf = nullptr;  // the four planes of the motion G-buffer, W*H*4 floats each
    float* d_tmp_f32 = nullptr;   // the accumulated frame (what the denoiser reads)
    uint8_t* d_tmp_u8 = nullptr;  // ... and its unorm8 image
    hipStream_t tmp_stream = nullptr;
    hipEvent_t tmp_ev[3] = {nullptr, nullptr, nullptr};
    int tmp_device = -1;
    std::vector<rt_renderer*> tile_handles;
    rt_comm* comm = nullptr;
    rt_stats last{};

    HipRendererBase(int kind, std::array<int32_t, 2> img_size, uint8_t* image, uint32_t max_depth, uint32_t sample_count)
        : img_size(img_size), image(image), max_depth(max_depth), sample_count(sample_count), kind(kind) {}
    ~HipRendererBase() override {
        for (rt_renderer* h : tile_handles) rt_renderer_destroy(h);
        rt_comm_destroy(comm);
        rt_renderer_destroy(handle);
        release_denoiser();
        release_accumulator();
    }

    // the accumulator's defaults (rtamd/renderer.py: TEMPORAL_*)
    static constexpr float kTemporalPositionFraction = 0.05f, kTemporalCosNormal = 0.9f;
    // the denoiser's defaults (rtamd/renderer.py: DENOISE_*): sigma_position is a fraction of the largest extent of the scene's bounds
    static constexpr float kSigmaColor = 1.0f, kSigmaNormal = 0.25f, kPositionFraction = 0.05f, kSigmaAlbedo = 0.1f;
    static constexpr uint32_t kMinHistory = 4; // DENOISE_MIN_HISTORY

    static void hip_check(hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    }
    void release_denoiser() {
        if (den_device >= 0 && hipSetDevice(den_device) == hipSuccess) {
            if (den_stream) (void)hipStreamSynchronize(den_stream), (void)hipStreamDestroy(den_stream);
            for (hipEvent_t& e : den_ev)
                if (e) (void)hipEventDestroy(e), e = nullptr;
            (void)hipFree(d_gbuf), (void)hipFree(d_den_u8), (void)hipFree(d_var);
        }
        rt_denoiser_destroy(denoiser);
        denoiser = nullptr, d_gbuf = nullptr, d_den_u8 = nullptr, d_var = nullptr, den_stream = nullptr, den_device = -1;
    }

    void release_accumulator() {
        if (tmp_device >= 0 && hipSetDevice(tmp_device) == hipSuccess) {
            if (tmp_stream) (void)hipStreamSynchronize(tmp_stream), (void)hipStreamDestroy(tmp_stream);
            for (hipEvent_t& e : tmp_ev)
                if (e) (void)hipEventDestroy(e), e = nullptr;
            (void)hipFree(d_tmp_gbuf), (void)hipFree(d_tmp_f32), (void)hipFree(d_tmp_u8), (void)hipFree(d_tmp_mom), (void)hipFree(d_tmp_len);
        }
        rt_temporal_destroy(accumulator);
        accumulator = nullptr, d_tmp_gbuf = nullptr, d_tmp_f32 = nullptr, d_tmp_u8 = nullptr, d_tmp_mom = nullptr, d_tmp_len = nullptr;
        tmp_stream = nullptr, tmp_device = -1;
    }

    static float scene_scale(rt_scene* sc) { // the largest extent of the scene's bounds (rtamd/renderer.py: Scene.scale)
        rt_scene_info_t info{};
        rt_check(rt_scene_info(sc, &info));
        float scale = 0.0f;
        for (int a = 0; a < 3; ++a) scale = std::max(scale, info.bounds_hi[a] - info.bounds_lo[a]);
        return scale;
    }

    // d_frame (this frame's fp32 image, W x H, on `dev`) accumulated over the frames before it; returns the accumulated fp32 frame (on the device)
    // and leaves its unorm8 image in `image`. Prints the device time of the motion G-buffer and of the accumulation (hipEvents on one stream).
    const float* accumulate_image(const Camera& camera, rt_scene* sc, int dev, const void* d_frame) {
        const size_t n = (size_t)img_size[0] * (size_t)img_size[1];
        hip_check(hipSetDevice(dev), "hipSetDevice");
        if (!accumulator) {
            tmp_device = dev;
            const bool moments = denoise && guided > 0.0f;
            rt_check(rt_temporal_create_ex(dev, img_size[0], img_size[1], moments ? RT_TEMPORAL_MOMENTS : 0u, &accumulator));
            if (moments) {
                hip_check(hipMalloc((void**)&d_tmp_mom, n * 8), "hipMalloc");
                hip_check(hipMalloc((void**)&d_tmp_len, n * 4), "hipMalloc");
            }
            hip_check(hipMalloc((void**)&d_tmp_gbuf, 4 * n * 16), "hipMalloc");
            hip_check(hipMalloc((void**)&d_tmp_f32, n * 16), "hipMalloc");
            hip_check(hipMalloc((void**)&d_tmp_u8, n * 4), "hipMalloc");
            hip_check(hipStreamCreateWithFlags(&tmp_stream, hipStreamNonBlocking), "hipStreamCreate");
            for (hipEvent_t& e : tmp_ev) hip_check(hipEventCreate(&e), "hipEventCreate");
        }
        const rt_temporal_params p{temporal, kTemporalPositionFraction * scene_scale(sc), kTemporalCosNormal};
        float* g = d_tmp_gbuf;
        hip_check(hipEventRecord(tmp_ev[0], tmp_stream), "hipEventRecord");
        rt_check(rt_scene_gbuffer_motion_device(sc, &camera.c, g, g + 4 * n, g + 8 * n, g + 12 * n, tmp_stream));
        hip_check(hipEventRecord(tmp_ev[1], tmp_stream), "hipEventRecord");
        if (d_tmp_mom)
            rt_check(rt_temporal_accumulate_moments_device(accumulator, &p, &camera.c, d_frame, g + 4 * n, g + 8 * n, g + 12 * n, d_tmp_f32, d_tmp_u8,
                                                           d_tmp_len, d_tmp_mom, tmp_stream));
        else
            rt_check(rt_temporal_accumulate_device(accumulator, &p, &camera.c, d_frame, g + 4 * n, g + 8 * n, g + 12 * n, d_tmp_f32, d_tmp_u8, nullptr, tmp_stream));
        hip_check(hipEventRecord(tmp_ev[2], tmp_stream), "hipEventRecord");
        hip_check(hipStreamSynchronize(tmp_stream), "hipStreamSynchronize");
        float g_ms = 0.0f, a_ms = 0.0f;
        hip_check(hipEventElapsedTime(&g_ms, tmp_ev[0], tmp_ev[1]), "hipEventElapsedTime");
        hip_check(hipEventElapsedTime(&a_ms, tmp_ev[1], tmp_ev[2]), "hipEventElapsedTime");
        hip_check(hipMemcpy(image, d_tmp_u8, n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
        std::printf("Temporal: max history %u, motion G-buffer %.3f ms, accumulation %.3f ms on device %d\n", temporal, g_ms, a_ms, dev);
        return d_tmp_f32;
    }

    // d_frame (the last pass's fp32 frame, W x H, on `dev`) -> `image`, denoised with the G-buffer of `sc` (the scene on `dev`); prints the device
    // time of the G-buffer and of the filter (hipEvents on one stream). The frame is complete when this is called: every render call before it returns
    // with its frame on the device.
    void denoise_image(const Camera& camera, rt_scene* sc, int dev, const void* d_frame) {
        const size_t n = (size_t)img_size[0] * (size_t)img_size[1];
        if (den_device != dev) release_denoiser();
        hip_check(hipSetDevice(dev), "hipSetDevice");
        if (!denoiser) {
            den_device = dev;
            rt_check(rt_denoiser_create_ex(dev, img_size[0], img_size[1], guided > 0.0f ? RT_DENOISER_VARIANCE : 0u, &denoiser));
            if (guided > 0.0f) hip_check(hipMalloc((void**)&d_var, n * 4), "hipMalloc");
            hip_check(hipMalloc((void**)&d_gbuf, 3 * n * 16), "hipMalloc");
            hip_check(hipMalloc((void**)&d_den_u8, n * 4), "hipMalloc");
            hip_check(hipStreamCreateWithFlags(&den_stream, hipStreamNonBlocking), "hipStreamCreate");
            for (hipEvent_t& e : den_ev) hip_check(hipEventCreate(&e), "hipEventCreate");
        }
        const float scale = scene_scale(sc);
        const rt_denoise_params p{denoise, kSigmaColor, kSigmaNormal, kPositionFraction * scale, kSigmaAlbedo};
        hip_check(hipEventRecord(den_ev[0], den_stream), "hipEventRecord");
        rt_check(rt_scene_gbuffer_device(sc, &camera.c, d_gbuf, d_gbuf + 4 * n, d_gbuf + 8 * n, den_stream));
        hip_check(hipEventRecord(den_ev[1], den_stream), "hipEventRecord");
        if (guided > 0.0f) {
            // (the moments belong to d_frame: both are this frame's rt_temporal_accumulate_moments_device outputs, complete when it returned)
            const rt_denoise_var_params vp{denoise, guided, kSigmaNormal, kPositionFraction * scale, kSigmaAlbedo, kMinHistory};
            rt_check(rt_denoise_variance_device(denoiser, &vp, d_frame, d_gbuf, d_gbuf + 4 * n, d_gbuf + 8 * n, temporal ? d_tmp_mom : nullptr,
                                                temporal ? d_tmp_len : nullptr, d_var, den_stream));
            hip_check(hipEventRecord(den_ev[3], den_stream), "hipEventRecord");
            rt_check(rt_denoise_guided_device(denoiser, &vp, d_frame, d_gbuf, d_gbuf + 4 * n, d_gbuf + 8 * n, d_var, nullptr, d_den_u8, nullptr, den_stream));
        } else
            rt_check(rt_denoise_device(denoiser, &p, d_frame, d_gbuf, d_gbuf + 4 * n, d_gbuf + 8 * n, nullptr, d_den_u8, den_stream));
        hip_check(hipEventRecord(den_ev[2], den_stream), "hipEventRecord");
        hip_check(hipStreamSynchronize(den_stream), "hipStreamSynchronize");
        float g_ms = 0.0f, f_ms = 0.0f, v_ms = 0.0f;
        hip_check(hipEventElapsedTime(&g_ms, den_ev[0], den_ev[1]), "hipEventElapsedTime");
        hip_check(hipEventElapsedTime(&f_ms, guided > 0.0f ? den_ev[3] : den_ev[1], den_ev[2]), "hipEventElapsedTime");
        if (guided > 0.0f) hip_check(hipEventElapsedTime(&v_ms, den_ev[1], den_ev[3]), "hipEventElapsedTime");
        hip_check(hipMemcpy(image, d_den_u8, n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
        if (guided > 0.0f)
            std::printf("Denoise: %u iterations, G-buffer %.3f ms, variance %.3f ms, filter %.3f ms on device %d\n", denoise, g_ms, v_ms, f_ms, dev);
        else
            std::printf("Denoise: %u iterations, G-buffer %.3f ms, filter %.3f ms on device %d\n", denoise, g_ms, f_ms, dev);
    }

    // one frame over devices.size() tiles: returns with `image` assembled and `last` = summed rays / wall time
    void render_tiled(const Camera& camera, const Scene& scene) {
        const uint32_t G = (uint32_t)devices.size();
        if (tile_handles.empty() || bound != &scene) {
            for (rt_renderer* h : tile_handles) rt_renderer_destroy(h);
            tile_handles.assign(G, nullptr);
            for (uint32_t k = 0; k < G; ++k) {
                rt_check(rt_renderer_create(kind, scene.on_device(devices[k]), img_size[0], img_size[1], max_depth, sample_count,
                                            RT_SEED_DEFAULT, &tile_handles[k]));
                rt_check(rt_renderer_set_tile(tile_handles[k], k, G, 8));
                if (has_schedule) rt_check(rt_renderer_set_schedule(tile_handles[k], &schedule));
            }
            bound = &scene;
        }
        if (!comm) {
            rt_check(rt_comm_create((int)G, devices.data(), &comm));
            std::printf("Tile gather: %s\n", rt_comm_uses_rccl(comm) ? "RCCL ncclGather over xGMI" : "device copies (a device is listed twice: no RCCL rank per tile)");
        }
        std::vector<rt_stats> st(G);
        std::vector<std::string> err(G);
        std::vector<std::thread> threads;
        const auto t0 = std::chrono::high_resolution_clock::now();
        for (uint32_t k = 0; k < G; ++k) {
            threads.emplace_back([&, k]() {
                rt_renderer* h = tile_handles[k];
                if (rt_renderer_set_russian_roulette(h, russian_roulette) != RT_OK || (passes > 1 && rt_renderer_set_progressive(h, 1) != RT_OK) ||
                    rt_render_frame_begin(h, &camera.c, denoise ? rt_renderer_tile_f32(h) : nullptr, rt_renderer_tile_u8(h), nullptr) != RT_OK ||
                    rt_render_frame_end(h, &st[k]) != RT_OK) {
                    err[k] = rt_last_error(); // rt_last_error is per thread
                    return;
                }
                for (uint32_t p = 1; p < passes; ++p) { // every rank continues its own strips, into its own tile buffer
                    rt_stats more{};
                    void* f32 = denoise ? rt_renderer_tile_f32(h) : nullptr;
                    const int rc = adaptive >= 0.0f ? rt_render_frame_continue_adaptive_device(h, sample_count, adaptive, min_samples, f32,
                                                                                                 rt_renderer_tile_u8(h), nullptr, &more, nullptr)
                                                    : rt_render_frame_continue_device(h, sample_count, f32, rt_renderer_tile_u8(h), nullptr, &more);
                    if (rc != RT_OK) {
                        err[k] = rt_last_error();
                        return;
                    }
                    add_stats(st[k], more);
                }
            });
        }
        for (auto& t : threads) t.join();
        for (uint32_t k = 0; k < G; ++k)
            if (!err[k].empty()) throw std::runtime_error("librt_mi355x (tile " + std::to_string(k) + "): " + err[k]);
        rt_check(rt_frame_gather(comm, tile_handles.data(), nullptr, image, denoise ? 1 : 0, 0)); // strips -> root GPU -> full frame -> host, once
        const double wall = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        last = rt_stats{};
        for (uint32_t k = 0; k < G; ++k) {
            last.rays += st[k].rays;
            last.launches += st[k].launches;
            last.device_ms = std::max(last.device_ms, st[k].device_ms);
        }
        last.seconds = wall;
    }

    // a continuation's statistics added to the frame's: what the stat lines report for all the passes together
    static void add_stats(rt_stats& into, const rt_stats& more) {
        into.rays += more.rays;
        into.launches += more.launches;
        into.seconds += more.seconds;
        into.device_ms += more.device_ms;
    }

    void render_frame(const Camera& camera, const Scene& scene) override {
        if (devices.size() > 1) {
            if (kind == RT_RENDERER_WAVEFRONT)
                for (uint32_t s = 0; s < sample_count * passes; ++s) std::printf("Sample %u\n", s);
            render_tiled(camera, scene);
            if (denoise) denoise_image(camera, scene.on_device(devices[0]), devices[0], rt_comm_frame_f32(comm)); // the root's frame and scene
            report_and_write(last.seconds); // tiles run concurrently: the frame time is the wall time of the slowest
            return;
        }
        if (!handle || bound != &scene) { // the ray queues belong to a scene's device: created on first use
            rt_renderer_destroy(handle);
            handle = nullptr;
            rt_check(rt_renderer_create(kind, scene.handle, img_size[0], img_size[1], max_depth, sample_count, RT_SEED_DEFAULT, &handle));
            if (has_schedule) rt_check(rt_renderer_set_schedule(handle, &schedule));
            bound = &scene;
        }
        rt_check(rt_renderer_set_russian_roulette(handle, russian_roulette));
        if (temporal) rt_check(rt_renderer_set_frame_seed(handle, frame_salt));
        if (passes > 1) rt_check(rt_renderer_set_progressive(handle, 1));
        if (kind == RT_RENDERER_WAVEFRONT)
            for (uint32_t s = 0; s < sample_count * passes; ++s) std::printf("Sample %u\n", s); // src/render_wavefront.cpp:402
        // (a host fp32 pointer makes the renderer write its own device copy of the frame, rt_renderer_tile_f32, which the denoiser reads)
        if (denoise || temporal) frame_f32.resize((size_t)img_size[0] * (size_t)img_size[1] * 4);
        float* f32 = denoise || temporal ? frame_f32.data() : nullptr;
        rt_check(rt_render_frame(handle, &camera.c, f32, image, &last));
        for (uint32_t p = 1; p < passes; ++p) { // the image of the last pass holds all sample_count x passes samples
            rt_stats more{};
            if (adaptive >= 0.0f) rt_check(rt_render_frame_continue_adaptive(handle, sample_count, adaptive, min_samples, f32, image, &more, nullptr));
            else rt_check(rt_render_frame_continue(handle, sample_count, f32, image, &more));
            add_stats(last, more);
        }
        const void* d_frame = rt_renderer_tile_f32(handle); // the renderer's own copy of the frame
        if (temporal) d_frame = accumulate_image(camera, scene.handle, scene.device, d_frame);
        if (denoise) denoise_image(camera, scene.handle, scene.device, d_frame);
        report_and_write(last.device_ms * 1e-3);
    }

    void report_and_write(double secs) {
        const double rays_per_sec = secs > 0 ? (double)last.rays / secs : 0.0;
        // the three lines benchmark.py scrapes (src/render_wavefront.cpp:425-427, benchmark.py:49-55)
        std::printf("Time measured: %.6f seconds\n", secs);
        std::printf("Total rays: %llu\n", (unsigned long long)last.rays);
        std::printf("Rays/sec: %.2fM\n", rays_per_sec / 1000000.0);
        if (has_schedule && devices.size() <= 1) // what ran (rt_stats): launches of the traversal kernels of the frame
            std::printf("Schedule: %u stream lanes, launches: extend %u, shade %u, shoot %u, finish %u\n", last.stream_lanes, last.launches_by_kernel[RT_K_WF_EXTEND],
                        last.launches_by_kernel[RT_K_WF_SHADE], last.launches_by_kernel[RT_K_WF_SHOOT], last.launches_by_kernel[RT_K_WF_FINISH]);
        std::printf("Writing image to disk\n");
        if (!rthost::write_png_rgba8(out_path.c_str(), (uint32_t)img_size[0], (uint32_t)img_size[1], image, (size_t)img_size[0] * 4)) {
            std::printf("Failed to write image to disk.\n"); // src/util.hpp:27-30
            throw std::runtime_error("cannot write " + out_path);
        }
    }
};

struct MegakernelRenderer : public HipRendererBase {
    MegakernelRenderer(std::array<int32_t, 2> img_size, uint8_t* image, uint32_t max_depth, uint32_t sample_count)
        : HipRendererBase(RT_RENDERER_MEGAKERNEL, img_size, image, max_depth, sample_count) {}
};

struct WavefrontRenderer : public HipRendererBase {
    WavefrontRenderer(std::array<int32_t, 2> img_size, uint8_t* image, uint32_t max_depth, uint32_t sample_count)
        : HipRendererBase(RT_RENDERER_WAVEFRONT, img_size, image, max_depth, sample_count) {}
};

} // namespace raytracer
