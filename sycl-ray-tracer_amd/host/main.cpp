// main.cpp — the `raytracer` CLI with the reference's flags (src/main.cpp:8-77) on the MI355X path.
//
//   -d,--max-depth N       (10)       -s,--sample-count N  (32)      scene_path (./assets/sponza.glb)
//   -w,--wavefront         -m,--megakernel        neither => wavefront
// Extensions (the reference hard-codes 1920x1080, one device, out.png):
//   --width N --height N   --device N   --devices A,B,..   --out FILE   --bvh {sah,lbvh}   --rr N   --quiet
//   --passes K             render -s samples, then continue the frame K - 1 times by -s samples (progressive rendering): the image of
//                          K x -s samples, bit for bit; the statistics lines sum the passes' rays and times
//   --adaptive T [--min-samples N]   with --passes: passes 2 .. K continue only the 8x8 blocks that are still noisy (adaptive sampling:
//                          rt_render_frame_continue_adaptive, threshold T on the two-image error, blocks under N samples always continue)
//   --schedule {default,per-sample,per-bounce,per-bounce-fused}   which of the wavefront renderer's schedules renders the frame
//   --denoise ITER         every image written is denoised after its last pass (rt_scene_gbuffer + rt_denoise, ITER a-trous iterations,
//                          the default sigmas of rtamd/renderer.py); a tiled frame is denoised on the root device after the gather
//   --guided SIGMA_L       with --denoise: the variance-guided filter in rt_denoise's place (rt_denoise_variance + rt_denoise_guided,
//                          sigma_luminance = SIGMA_L standard deviations; 4 is rtamd/renderer.py's default). With --temporal the variance comes
//                          from the accumulated luminance moments where the history is at least 4 frames, else from a 7 x 7 window
//   --temporal N           with --frames: temporal accumulation. Frame f is rendered with seed salt f (rt_renderer_set_frame_seed), then
//                          accumulated over the frames before it by reprojection (rt_scene_gbuffer_motion + rt_temporal_accumulate, history
//                          capped at N frames), then denoised if --denoise is given, then written. One device only.
//   --frames N --spin DEG  render N frames, every instance turned by DEG more per frame about the vertical axis through the centre of the
//                          scene's bounds (rt_scene_update between frames: the BVH is refit, not rebuilt); writes OUT_0000.png onwards
//                          (rt_renderer_set_schedule; per-bounce = the reference's own: src/render_wavefront.cpp:396-417)
// Prints the same lines as the reference (Loading scene, loader chatter, Sample n, the three statistics
// lines benchmark.py scrapes, Writing image to disk) and writes the PNG.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "renderer.h"

static void usage(const char* argv0) {
    std::printf("Usage: %s [OPTIONS] [scene_path]\n\n"
                "Options:\n"
                "  -h,--help                   Print this help message and exit\n"
                "  -d,--max-depth UINT         Max depth\n"
                "  -s,--sample-count UINT      Sample count\n"
                "  -w,--wavefront              Use wavefront renderer\n"
                "  -m,--megakernel             Use megakernel renderer\n"
                "  --width UINT --height UINT  Image size (default 1920x1080)\n"
                "  --device INT                HIP device (default 0)\n"
                "  --devices A,B,...           tile the frame over these HIP devices (8-row strips, one host thread each)\n"
                "  --out FILE                  Output PNG (default out.png)\n"
                "  --bvh sah|lbvh              BVH builder (default sah)\n"
                "  --rr UINT                   Russian roulette from this bounce on (default 0 = off, as the reference)\n"
                "  --passes UINT               progressive rendering: -s samples, then K - 1 continuations by -s samples (default 1)\n"
                "  --adaptive FLOAT            adaptive sampling: passes 2 .. K continue only the 8x8 blocks whose two-image error is at\n"
                "                              least this threshold (default: off, every pass continues every pixel)\n"
                "  --min-samples UINT          with --adaptive: blocks with fewer samples always continue (default 0)\n"
                "  --schedule NAME             wavefront schedule: default (one launch per frame), per-sample, per-bounce (a launch pair per\n"
                "                              bounce with compaction in between, the reference's), per-bounce-fused (one kernel per bounce)\n"
                "  --frames UINT               render this many frames, written to OUT_0000.png onwards (default 1)\n"
                "  --spin FLOAT                with --frames: turn every instance by this many degrees per frame about the vertical axis\n"
                "                              through the centre of the scene (a BVH refit per frame; prints each update's device time)\n"
                "  --denoise UINT              denoise every image written with this many a-trous iterations (1 .. 10; default 0 = off),\n"
                "                              guided by the scene's primary-hit G-buffer (a tiled frame: on the first device, after the\n"
                "                              gather); prints the G-buffer's and the filter's device time\n"
                "  --guided FLOAT              with --denoise: filter with the variance-guided a-trous (the colour tolerance of every pixel is this\n"
                "                              many standard deviations of its luminance; 4 is the default of the Python interface); with\n"
                "                              --temporal the variance comes from the accumulated moments; adds the variance stage's device time\n"
                "  --temporal UINT             with --frames > 1: accumulate every frame over the frames before it by reprojection, the history\n"
                "                              capped at this many frames (1 .. 4096; default 0 = off); every frame gets its own noise (seed salt\n"
                "                              = frame number); before --denoise; one device only; prints the stage's device times\n"
                "  --quiet                     No loader chatter\n"
                "\nThe camera must lie within 100 scene scales of the scene's bounds (scale = largest extent or coordinate): farther out the\n"
                "conservative box culling of the closest-hit query no longer holds and the frame is refused with an error, not rendered wrong.\n",
                argv0);
}

int main(int argc, const char* argv[]) {
    uint32_t max_depth = 10, sample_count = 32, rr = 0, passes = 1, min_samples = 0, frames = 1, denoise = 0, temporal = 0;
    float adaptive = -1.0f; // < 0: off
    float guided = 0.0f;    // 0: off
    double spin = 0.0;      // degrees per frame (--frames)
    std::string scene_path = "./assets/sponza.glb", out_path = "out.png";
    bool use_wavefront = false, use_megakernel = false, quiet = false;
    int32_t width = 1920, height = 1080;
    int device = 0, bvh = RT_BVH_DEFAULT;
    std::vector<int> devices;
    bool have_scene = false;
    rt_schedule schedule{0u, 0u, 0u, -1, 0u, 0u, -1, 0u, 0u, -1}; // the library's default
    bool schedule_given = false;

    auto need = [&](int& i) -> const char* {
        if (i + 1 >= argc) {
            std::fprintf(stderr, "%s: 1 required TEXT missing\n", argv[i]);
            std::exit(106);
        }
        return argv[++i];
    };
    auto to_u32 = [&](const char* flag, const char* v) -> uint32_t {
        char* end = nullptr;
        unsigned long x = std::strtoul(v, &end, 10);
        if (!*v || *end || v[0] == '-') {
            std::fprintf(stderr, "Could not convert: %s = %s\n", flag, v);
            std::exit(104);
        }
        return (uint32_t)x;
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-h" || a == "--help") { usage(argv[0]); return 0; }
        else if (a == "-d" || a == "--max-depth") max_depth = to_u32("--max-depth", need(i));
        else if (a.rfind("--max-depth=", 0) == 0) max_depth = to_u32("--max-depth", a.c_str() + 12);
        else if (a == "-s" || a == "--sample-count") sample_count = to_u32("--sample-count", need(i));
        else if (a.rfind("--sample-count=", 0) == 0) sample_count = to_u32("--sample-count", a.c_str() + 15);
        else if (a == "-w" || a == "--wavefront") use_wavefront = true;
        else if (a == "-m" || a == "--megakernel") use_megakernel = true;
        else if (a == "--width") width = (int32_t)to_u32("--width", need(i));
        else if (a == "--height") height = (int32_t)to_u32("--height", need(i));
        else if (a == "--device") device = (int)to_u32("--device", need(i));
        else if (a == "--devices") {
            const std::string v = need(i);
            size_t pos = 0;
            while (pos <= v.size()) {
                const size_t comma = v.find(',', pos);
                const std::string tok = v.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
                devices.push_back((int)to_u32("--devices", tok.c_str()));
                if (comma == std::string::npos) break;
                pos = comma + 1;
            }
        }
        else if (a == "--out") out_path = need(i);
        else if (a == "--rr") rr = to_u32("--rr", need(i));
        else if (a == "--passes") {
            passes = to_u32("--passes", need(i));
            if (passes == 0) { std::fprintf(stderr, "--passes: expected at least 1\n"); return 105; }
        }
        else if (a == "--adaptive") {
            const std::string v = need(i);
            char* end = nullptr;
            adaptive = std::strtof(v.c_str(), &end);
            if (v.empty() || *end || !(adaptive >= 0.0f)) { std::fprintf(stderr, "--adaptive: expected a threshold >= 0, got '%s'\n", v.c_str()); return 105; }
        }
        else if (a == "--min-samples") min_samples = to_u32("--min-samples", need(i));
        else if (a == "--denoise") {
            denoise = to_u32("--denoise", need(i));
            if (denoise > 10) { std::fprintf(stderr, "--denoise: expected 0 .. 10 iterations\n"); return 105; }
        }
        else if (a == "--guided") {
            const std::string v = need(i);
            char* end = nullptr;
            guided = std::strtof(v.c_str(), &end);
            if (v.empty() || *end || !(guided >= 1e-6f)) { std::fprintf(stderr, "--guided: expected a sigma of at least 1e-6 (inf = luminance ignored), got '%s'\n", v.c_str()); return 105; }
        }
        else if (a == "--temporal") {
            temporal = to_u32("--temporal", need(i));
            if (temporal > 4096) { std::fprintf(stderr, "--temporal: expected a history of 1 .. 4096 frames (0 = off)\n"); return 105; }
        }
        else if (a == "--quiet") quiet = true;
        else if (a == "--frames") {
            frames = to_u32("--frames", need(i));
            if (frames == 0) { std::fprintf(stderr, "--frames: expected at least 1\n"); return 105; }
        }
        else if (a == "--spin") {
            const std::string v = need(i);
            char* end = nullptr;
            spin = std::strtod(v.c_str(), &end);
            if (v.empty() || *end || !std::isfinite(spin)) { std::fprintf(stderr, "--spin: expected degrees, got '%s'\n", v.c_str()); return 105; }
        }
        else if (a == "--schedule") {
            const std::string v = need(i);
            schedule_given = true;
            if (v == "default") schedule_given = false;
            else if (v == "per-sample") schedule.samples_per_launch = 1;
            else if (v == "per-bounce") schedule.finish_depth = RT_SCHED_ALL_BOUNCES;
            else if (v == "per-bounce-fused") schedule.finish_depth = RT_SCHED_ALL_BOUNCES, schedule.fused_bounce = 1;
            else { std::fprintf(stderr, "--schedule: expected default, per-sample, per-bounce or per-bounce-fused\n"); return 105; }
        }
        else if (a == "--bvh") {
            const std::string v = need(i);
            if (v == "sah") bvh = RT_BVH_SAH;
            else if (v == "lbvh") bvh = RT_BVH_LBVH;
            else { std::fprintf(stderr, "--bvh: expected sah or lbvh\n"); return 105; }
        } else if (!a.empty() && a[0] == '-') {
            std::fprintf(stderr, "The following argument was not expected: %s\nRun with --help for more information.\n", a.c_str());
            return 109;
        } else if (!have_scene) {
            scene_path = a;
            have_scene = true;
        } else {
            std::fprintf(stderr, "The following argument was not expected: %s\n", a.c_str());
            return 109;
        }
    }
    if (!use_wavefront && !use_megakernel) use_wavefront = true; // src/main.cpp:26-28
    if (guided > 0.0f && !denoise) { std::fprintf(stderr, "--guided: goes with --denoise of at least 1 iteration\n"); return 105; }
    if (temporal && frames < 2) { std::fprintf(stderr, "--temporal: needs --frames of at least 2\n"); return 105; }
    if (temporal && devices.size() > 1) { std::fprintf(stderr, "--temporal: one device only (--devices with one entry)\n"); return 105; }

    std::printf("Loading scene: %s\n", scene_path.c_str());
    try {
        const int n_dev = rt_device_count();
        if (n_dev <= 0) throw std::runtime_error(std::string("no HIP device: ") + rt_last_error());
        for (int d : devices)
            if (d >= n_dev) throw std::runtime_error("--devices: HIP device " + std::to_string(d) + " does not exist");
        if (!devices.empty()) device = devices[0];
        if (devices.size() > 1) {
            std::printf("Running on devices:");
            for (int d : devices) std::printf(" %d", d);
            std::printf(" of %d (gfx950 path, frame tiled in 8-row strips)\n", n_dev);
        } else
            std::printf("Running on device: HIP device %d of %d (gfx950 path)\n", device, n_dev); // src/app.hpp:51-54
        std::vector<uint8_t> image_buf((size_t)width * (size_t)height * 4);
        if (frames > 1 && devices.size() > 1) throw std::runtime_error("--frames: one device only");
        raytracer::Scene scene(scene_path, device, bvh, !quiet, frames > 1 ? (temporal ? RT_SCENE_UPDATABLE | RT_SCENE_KEEP_PREVIOUS : RT_SCENE_UPDATABLE) : 0u);
        raytracer::Camera camera({width, height}, scene.camera_position, scene.camera_direction, scene.camera_focal_length);
        std::unique_ptr<raytracer::IRenderer> renderer;
        if (use_megakernel) {
            auto* r = new raytracer::MegakernelRenderer({width, height}, image_buf.data(), max_depth, sample_count);
            r->out_path = out_path;
            r->russian_roulette = rr;
            r->devices = devices;
            r->passes = passes;
            r->adaptive = adaptive, r->min_samples = min_samples;
            r->denoise = denoise;
            r->guided = guided;
            r->temporal = temporal;
            renderer.reset(r);
        } else {
            auto* r = new raytracer::WavefrontRenderer({width, height}, image_buf.data(), max_depth, sample_count);
            r->out_path = out_path;
            r->russian_roulette = rr;
            r->devices = devices;
            r->passes = passes;
            r->adaptive = adaptive, r->min_samples = min_samples;
            r->denoise = denoise;
            r->guided = guided;
            r->temporal = temporal;
            if (schedule_given) r->schedule = schedule, r->has_schedule = true;
            renderer.reset(r);
        }
        if (frames == 1) renderer->render_frame(camera, scene);
        const std::string stem = out_path.size() > 4 && out_path.compare(out_path.size() - 4, 4, ".png") == 0 ? out_path.substr(0, out_path.size() - 4) : out_path;
        for (uint32_t f = 0; frames > 1 && f < frames; ++f) {
            char name[32];
            std::snprintf(name, sizeof(name), "_%04u.png", f);
            static_cast<raytracer::HipRendererBase*>(renderer.get())->out_path = stem + name;
            static_cast<raytracer::HipRendererBase*>(renderer.get())->frame_salt = f; // (used with --temporal only)
            if (f > 0) {
                const rt_update_stats us = scene.spin(spin * (double)f);
                std::printf("Frame %u: update %.3f ms on the device (%u launches, %u nodes refit)\n", f, us.device_ms, us.launches, us.refit_nodes);
            }
            renderer->render_frame(camera, scene);
        }
    } catch (const std::exception& e) {
        std::printf("Caught exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
