// rt_probe_volume.hip — irradiance probe volumes: rt_probe_volume_create / _destroy, rt_probe_volume_entries[_device], _bake[_device],
// _set_sh[_device], _get_sh[_device], _sample[_device], and their kernels. A regular grid of probes over one scene, each holding nine
// spherical-harmonic coefficients (bands 0 to 2) of the radiance that arrives there, for lighting what has no parametrisation of its own.
// The bake is a composition around one path query (rt_path_query.hip, called through its public entry point), as the lightmap is around
// one gather query: the probes' entries, a uniform direction and a state each (k_pv_entries), the projection of the entries' radiances onto
// the basis (k_pv_project), and apart from the bake the trilinear interpolation and cosine-lobe evaluation at caller-supplied points
// (k_pv_sample). The arithmetic is the contract stated at rt_probe_volume_bake in include/rt_mi355x.h; the numpy model that pins it bit for
// bit is tests/test_probe_volume.py. No traversal, no LDS, no transcendental function and no float atomics in this unit: a coefficient is one
// lane's sequential sum, the statistics are ballots and integer sums.
#include "rt_internal.h"
#include "rt_device.h"

struct rt_probe_volume : CallBracket { // the host forms run on its stream
    rt_scene* scene = nullptr;
    rt_probe_volume_desc desc{};
    uint32_t probes = 0;
    float* d_pos = nullptr;          // 3 floats per entry (max_dirs entries per probe)
    float* d_dir = nullptr;          // 3 floats per entry: the fp32 direction the projection reads (the path query rounds its own copy to half)
    uint32_t* d_state = nullptr;     // per entry
    float* d_rad = nullptr;          // 3 floats per entry
    uint32_t* d_rays = nullptr;      // per entry
    float4* d_sh = nullptr;          // the table: 9 float4 per probe
    rt_probe_stats* d_stats = nullptr;
    float* d_host_pts = nullptr;     // the host form of sample: kPvStagePoints points at a time, pos | normal | rgb
    bool has_table = false;          // a bake or a set_sh was enqueued
};

namespace rt {

constexpr uint32_t kPvBlock = 256;      // k_pv_entries, k_pv_sample
constexpr uint32_t kPvStatBlock = 64;   // k_pv_project: one wave per workgroup, so a wave's ballot is the workgroup's count
constexpr uint32_t kPvTries = 8;        // pairs drawn at most for one direction
#ifndef RT_PV_SAMPLE_WAVES
#define RT_PV_SAMPLE_WAVES 4
#endif
constexpr uint32_t kPvSampleWaves = RT_PV_SAMPLE_WAVES; // waves per SIMD k_pv_sample's register budget allows (DESIGN.md §21 has the comparison)

// what the kernels read of a volume (rt_probe_volume_desc)
struct PvGrid {
    float origin[3], spacing[3];
    uint32_t count[3];
};

// Y_k(d), the nine real spherical harmonics of bands 0 to 2 in the contract's order and bracketing: one or more R1 operations each
RT_DEV float pv_Y(uint32_t k, float x, float y, float z) {
    switch (k) {
    case 0: return 0.2820948f;
    case 1: return __fmul_rn(0.48860252f, y);
    case 2: return __fmul_rn(0.48860252f, z);
    case 3: return __fmul_rn(0.48860252f, x);
    case 4: return __fmul_rn(1.0925485f, __fmul_rn(x, y));
    case 5: return __fmul_rn(1.0925485f, __fmul_rn(y, z));
    case 6: return __fmul_rn(0.31539157f, __fsub_rn(__fmul_rn(3.0f, __fmul_rn(z, z)), 1.0f));
    case 7: return __fmul_rn(1.0925485f, __fmul_rn(x, z));
    default: return __fmul_rn(0.54627424f, __fsub_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
    }
}

// Steps 1 and 2, one thread per entry e = p * dirs + j: the probe's position, a direction uniform on the sphere (Marsaglia 1972: a point of
// the unit disc by rejection, at most kPvTries pairs, the last pair pulled inside when all were rejected) and the state its draws leave.
// NULL outputs are not written.
__global__ void __launch_bounds__(kPvBlock) k_pv_entries(PvGrid G, uint32_t n, uint32_t dirs, uint32_t seed, float* __restrict__ pos_out,
                                                          float* __restrict__ dir_out, uint32_t* __restrict__ state_out) {
    const uint32_t e = blockIdx.x * kPvBlock + threadIdx.x; // below 2^31 (rt_probe_volume_create)
    if (e >= n) return;
    const uint32_t p = e / dirs;
    const uint32_t ix = p % G.count[0], iy = (p / G.count[0]) % G.count[1], iz = p / (G.count[0] * G.count[1]);
    uint32_t a = seed + (e + 1u) * 0x9E3779B9u;
    a = a ? a : 0x9E3779B9u;
    float x1 = 0.0f, x2 = 0.0f, s = 2.0f;
    for (uint32_t t = 0; t < kPvTries && !(s < 1.0f); ++t) {
        x1 = __fadd_rn(-1.0f, __fmul_rn(2.0f, rng_next(a)));
        x2 = __fadd_rn(-1.0f, __fmul_rn(2.0f, rng_next(a)));
        s = __fadd_rn(__fmul_rn(x1, x1), __fmul_rn(x2, x2));
    }
    if (!(s < 1.0f)) { // |x1|, |x2| <= 1, so s <= 1 now
        x1 = __fmul_rn(x1, 0.70710677f), x2 = __fmul_rn(x2, 0.70710677f);
        s = __fadd_rn(__fmul_rn(x1, x1), __fmul_rn(x2, x2));
    }
    const float r = __builtin_sqrtf(__fsub_rn(1.0f, s));
    if (pos_out) {
        pos_out[3 * (size_t)e] = __fadd_rn(G.origin[0], __fmul_rn((float)ix, G.spacing[0]));
        pos_out[3 * (size_t)e + 1] = __fadd_rn(G.origin[1], __fmul_rn((float)iy, G.spacing[1]));
        pos_out[3 * (size_t)e + 2] = __fadd_rn(G.origin[2], __fmul_rn((float)iz, G.spacing[2]));
    }
    if (dir_out) {
        dir_out[3 * (size_t)e] = __fmul_rn(__fmul_rn(2.0f, x1), r);
        dir_out[3 * (size_t)e + 1] = __fmul_rn(__fmul_rn(2.0f, x2), r);
        dir_out[3 * (size_t)e + 2] = __fsub_rn(1.0f, __fmul_rn(2.0f, s));
    }
    if (state_out) state_out[e] = a;
}

// Steps 4 and 5, one lane per (probe, coefficient), t = p * 9 + k, 64 consecutive t per wave: the lane sums its probe's directions in order
// and stores one float4 of the table. A probe is valid iff its first entry was not rejected (the path query rejects an entry by its origin,
// which a probe's entries share). The statistics: valid probes as a ballot of the k = 0 lanes, their entries' rays as a wave sum; lane 0
// adds them at the end.
__global__ void __launch_bounds__(kPvStatBlock) k_pv_project(const float* __restrict__ dir, const float* __restrict__ rad,
                                                              const uint32_t* __restrict__ rays, uint32_t probes, uint32_t dirs,
                                                              float4* __restrict__ sh, rt_probe_stats* __restrict__ stats) {
    const uint32_t t = blockIdx.x * kPvStatBlock + threadIdx.x; // below 2^24 * 9 + 64
    bool counted = false;
    unsigned long long traced = 0;
    if (t < probes * 9u) {
        const uint32_t p = t / 9u, k = t % 9u;
        const size_t e0 = (size_t)p * dirs;
        const bool valid = rays[e0] != 0xFFFFFFFFu;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (valid) {
            float cx = 0.0f, cy = 0.0f, cz = 0.0f;
#pragma unroll 8 // the loads of eight directions in flight; the sums stay in order
            for (uint32_t j = 0; j < dirs; ++j) {
                const float* d = dir + 3 * (e0 + j);
                const float* r = rad + 3 * (e0 + j);
                const float y = pv_Y(k, d[0], d[1], d[2]);
                cx = __fadd_rn(cx, __fmul_rn(r[0], y)), cy = __fadd_rn(cy, __fmul_rn(r[1], y)), cz = __fadd_rn(cz, __fmul_rn(r[2], y));
            }
            const float w = 12.566371f / (float)dirs;
            o = make_float4(__fmul_rn(cx, w), __fmul_rn(cy, w), __fmul_rn(cz, w), k == 0u ? 1.0f : 0.0f);
            if (k == 0u) {
                counted = true;
                for (uint32_t j = 0; j < dirs; ++j) traced += rays[e0 + j];
            }
        }
        sh[t] = o;
    }
    const uint32_t n_valid = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(counted));
    for (int off = 32; off > 0; off >>= 1) traced += __shfl_xor(traced, off, 64);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) stats->probes = probes; // the other two words were zeroed on the stream and are only added to
        if (n_valid) atomicAdd(&stats->valid, n_valid);
        if (traced) atomicAdd((unsigned long long*)&stats->rays, traced);
    }
}

// One axis of step 6: the cell and the two weights of coordinate q
struct PvAxis {
    uint32_t i0;
    float w0, w1;
};
RT_DEV PvAxis pv_axis(float q, float origin, float spacing, uint32_t count) {
    float g = __fsub_rn(q, origin) / spacing;
    g = __builtin_fminf(__builtin_fmaxf(g, 0.0f), (float)(count - 1u));
    const int32_t i = (int32_t)g, top = (int32_t)count - 2;
    const uint32_t i0 = count == 1u ? 0u : (uint32_t)(i < top ? i : top);
    const float f = __fsub_rn(g, (float)i0);
    return {i0, __fsub_rn(1.0f, f), f};
}

// Step 6, one thread per point: the eight corners of the point's cell, z outer, y, x inner; a corner is its probe's nine float4, contiguous
// (144 bytes), the validity in .w of the first. The nine loads of a corner are issued before its validity is looked at, so that the loads of
// the eight corners do not wait for one another; what an invalid probe holds is zeros and is not added.
__global__ void __launch_bounds__(kPvBlock, kPvSampleWaves) k_pv_sample(PvGrid G, const float4* __restrict__ sh, uint32_t n, const float* __restrict__ pos,
                                                         const float* __restrict__ nrm, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kPvBlock + threadIdx.x;
    if (i >= n) return;
    const float px = pos[3 * (size_t)i], py = pos[3 * (size_t)i + 1], pz = pos[3 * (size_t)i + 2];
    const float nx = nrm[3 * (size_t)i], ny = nrm[3 * (size_t)i + 1], nz = nrm[3 * (size_t)i + 2];
    float* o = out + 3 * (size_t)i;
    if (!(__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz) && __builtin_isfinite(nx) && __builtin_isfinite(ny) &&
          __builtin_isfinite(nz))) {
        o[0] = o[1] = o[2] = __uint_as_float(0x7FC00000u);
        return;
    }
    const PvAxis ax = pv_axis(px, G.origin[0], G.spacing[0], G.count[0]);
    const PvAxis ay = pv_axis(py, G.origin[1], G.spacing[1], G.count[1]);
    const PvAxis az = pv_axis(pz, G.origin[2], G.spacing[2], G.count[2]);
    float W = 0.0f, S[9][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k][0] = S[k][1] = S[k][2] = 0.0f;
#pragma unroll
    for (uint32_t dz = 0; dz < 2; ++dz) {
        if (dz && G.count[2] == 1u) continue;
#pragma unroll
        for (uint32_t dy = 0; dy < 2; ++dy) {
            if (dy && G.count[1] == 1u) continue;
#pragma unroll
            for (uint32_t dx = 0; dx < 2; ++dx) {
                if (dx && G.count[0] == 1u) continue;
                const uint32_t p = ((az.i0 + dz) * G.count[1] + (ay.i0 + dy)) * G.count[0] + (ax.i0 + dx); // inside the grid: i0 + 1 <= count - 1
                const float4* c = sh + 9 * (size_t)p;
                float4 v[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) v[k] = c[k];
                if (v[0].w == 0.0f) continue;
                const float w = __fmul_rn(__fmul_rn(dx ? ax.w1 : ax.w0, dy ? ay.w1 : ay.w0), dz ? az.w1 : az.w0);
                W = __fadd_rn(W, w);
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    S[k][0] = __fadd_rn(S[k][0], __fmul_rn(w, v[k].x));
                    S[k][1] = __fadd_rn(S[k][1], __fmul_rn(w, v[k].y));
                    S[k][2] = __fadd_rn(S[k][2], __fmul_rn(w, v[k].z));
                }
            }
        }
    }
    float E[3] = {0.0f, 0.0f, 0.0f};
    if (W != 0.0f) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float B = k == 0 ? 1.0f : (k < 4 ? 0.6666667f : 0.25f);
            const float y = pv_Y((uint32_t)k, nx, ny, nz);
#pragma unroll
            for (int c = 0; c < 3; ++c) E[c] = __fadd_rn(E[c], __fmul_rn(__fmul_rn(B, S[k][c] / W), y));
        }
    }
    o[0] = __builtin_fmaxf(E[0], 0.0f), o[1] = __builtin_fmaxf(E[1], 0.0f), o[2] = __builtin_fmaxf(E[2], 0.0f);
}

} // namespace rt

namespace {

static_assert(sizeof(rt_probe_volume_desc) == 40 && sizeof(rt_probe_bake_params) == 16 && sizeof(rt_probe_stats) == 16,
              "include/rt_mi355x.h states the sizes");

constexpr uint32_t kMaxCount = 256, kMaxDirs = 65536;
constexpr uint32_t kPvStagePoints = 65536; // points the host form of sample stages at a time: 36 bytes each

PvGrid grid_of(const rt_probe_volume* v) {
    PvGrid g{};
    std::memcpy(g.origin, v->desc.origin, 12), std::memcpy(g.spacing, v->desc.spacing, 12), std::memcpy(g.count, v->desc.count, 12);
    return g;
}

int check_bake_params(const rt_probe_volume* v, const rt_probe_bake_params* p) {
    if (!v || !p) return fail(RT_ERR_INVALID, "null argument");
    if (p->dirs == 0) return fail(RT_ERR_INVALID, "dirs must be at least 1");
    if (p->dirs > v->desc.max_dirs) return fail(RT_ERR_INVALID, "dirs exceeds the max_dirs the volume was created with");
    if (p->max_depth == 0) return fail(RT_ERR_INVALID, "max_depth must be at least 1");
    return RT_OK;
}

// the end of a host form whose copies lie inside the bracket: the call's end, then the stream has run dry
int end_call_host(rt_probe_volume* v) {
    if (const int rc = end_call(v, v->stream)) return rc;
    HIPCHK(hipStreamSynchronize(v->stream));
    return RT_OK;
}

// steps 1 and 2 on st into device pointers, any of them null. PRE: the call's bracket is open
int enqueue_entries(rt_probe_volume* v, const rt_probe_bake_params* p, float* pos, float* dir, uint32_t* state, hipStream_t st) {
    const uint32_t n = v->probes * p->dirs;
    hipLaunchKernelGGL(k_pv_entries, dim3((n + kPvBlock - 1u) / kPvBlock), dim3(kPvBlock), 0, st, grid_of(v), n, p->dirs, p->seed, pos, dir, state);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// rt_probe_volume_bake[_device]: the whole chain on st; the table stays in d_sh. out / stats: device pointers or null. PRE: the arguments were checked
int bake_enqueue(rt_probe_volume* v, const rt_probe_bake_params* p, float4* out, rt_probe_stats* stats, hipStream_t st) {
    if (const int rc = begin_call(v, st)) return rc;
    if (const int rc = enqueue_entries(v, p, v->d_pos, v->d_dir, v->d_state, st)) return rc;
    rt_path_query q{};
    q.n = v->probes * p->dirs, q.max_depth = p->max_depth, q.samples = 1, q.rr_start = p->rr_start;
    q.org = v->d_pos, q.dir = v->d_dir, q.rng = v->d_state, q.rng_out = nullptr, q.radiance = v->d_rad, q.rays = v->d_rays;
    if (const int rc = rt_trace_paths_device(v->scene, &q, st)) return rc; // records the scene's event for st
    HIPCHK(hipSetDevice(v->device));
    rt_probe_stats* d_stats = stats ? stats : v->d_stats;
    HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(rt_probe_stats), st));
    const uint32_t lanes = v->probes * 9u;
    hipLaunchKernelGGL(k_pv_project, dim3((lanes + kPvStatBlock - 1u) / kPvStatBlock), dim3(kPvStatBlock), 0, st, (const float*)v->d_dir,
                       (const float*)v->d_rad, (const uint32_t*)v->d_rays, v->probes, p->dirs, v->d_sh, d_stats);
    HIPCHK(hipGetLastError());
    if (out) HIPCHK(hipMemcpyAsync(out, v->d_sh, (size_t)v->probes * 144u, hipMemcpyDeviceToDevice, st));
    v->has_table = true;
    return end_call(v, st);
}

int sample_check(const rt_probe_volume* v, uint32_t n, const void* pos, const void* nrm, const void* out) {
    if (!v) return fail(RT_ERR_INVALID, "null argument");
    if (n && (!pos || !nrm || !out)) return fail(RT_ERR_INVALID, "null pos, normal or output");
    if (!v->has_table) return fail(RT_ERR_INVALID, "the volume holds no table yet: sample needs a bake or a set_sh first");
    return RT_OK;
}

// k_pv_sample over n device points on st. PRE: the call's bracket is open, n > 0
int enqueue_sample(rt_probe_volume* v, uint32_t n, const float* pos, const float* nrm, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_pv_sample, dim3((n + kPvBlock - 1u) / kPvBlock), dim3(kPvBlock), 0, st, grid_of(v), (const float4*)v->d_sh, n, pos, nrm, out);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

} // namespace

extern "C" {

int rt_probe_volume_create(rt_scene* s, const rt_probe_volume_desc* d, uint32_t flags, rt_probe_volume** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (!s) return fail(RT_ERR_INVALID, "null scene");
    if (!d) return fail(RT_ERR_INVALID, "null description");
    for (int a = 0; a < 3; ++a)
        if (d->count[a] < 1 || d->count[a] > kMaxCount) return fail(RT_ERR_INVALID, "every count must be 1 .. 256");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(d->spacing[a]) || !(d->spacing[a] > 0.0f)) return fail(RT_ERR_INVALID, "every spacing must be finite and above 0");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(d->origin[a])) return fail(RT_ERR_INVALID, "the origin must be finite");
    if (d->max_dirs < 1 || d->max_dirs > kMaxDirs) return fail(RT_ERR_INVALID, "max_dirs must be 1 .. 65536");
    const uint64_t probes = (uint64_t)d->count[0] * d->count[1] * d->count[2];
    if (probes * d->max_dirs > 0x7fffffffull) return fail(RT_ERR_INVALID, "too many entries (probes x max_dirs must stay below 2^31)");
    if (flags) return fail(RT_ERR_INVALID, "unknown probe volume flag");
    if (s->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    HIPCHK(hipSetDevice(s->device));
    return no_throw([&]() -> int {
        rt_probe_volume* v = new rt_probe_volume;
        v->scene = s, v->device = s->device, v->desc = *d, v->probes = (uint32_t)probes;
        const size_t e = (size_t)probes * d->max_dirs;
        if (hipMalloc((void**)&v->d_pos, e * 12u) != hipSuccess || hipMalloc((void**)&v->d_dir, e * 12u) != hipSuccess ||
            hipMalloc((void**)&v->d_state, e * 4u) != hipSuccess || hipMalloc((void**)&v->d_rad, e * 12u) != hipSuccess ||
            hipMalloc((void**)&v->d_rays, e * 4u) != hipSuccess || hipMalloc((void**)&v->d_sh, (size_t)probes * 144u) != hipSuccess ||
            hipMalloc((void**)&v->d_stats, sizeof(rt_probe_stats)) != hipSuccess ||
            hipMalloc((void**)&v->d_host_pts, (size_t)kPvStagePoints * 36u) != hipSuccess) {
            rt_probe_volume_destroy(v);
            return fail(RT_ERR_OOM, "hipMalloc of the probe volume's buffers failed");
        }
        if (const int rc = bracket_open(v)) {
            rt_probe_volume_destroy(v);
            return rc;
        }
        *out = v;
        return (int)RT_OK;
    });
}

void rt_probe_volume_destroy(rt_probe_volume* v) {
    if (!v) return;
    if (bracket_close(v))
        for (void* p : {(void*)v->d_pos, (void*)v->d_dir, (void*)v->d_state, (void*)v->d_rad, (void*)v->d_rays, (void*)v->d_sh, (void*)v->d_stats,
                        (void*)v->d_host_pts})
            (void)hipFree(p);
    delete v;
}

int rt_probe_volume_entries(rt_probe_volume* v, const rt_probe_bake_params* p, float* pos, float* dir, uint32_t* state) {
    if (const int rc = check_bake_params(v, p)) return rc;
    if (!pos && !dir && !state) return fail(RT_ERR_INVALID, "pos, dir and state are all null");
    hipStream_t st = v->stream;
    if (const int rc = begin_call(v, st)) return rc;
    if (const int rc = enqueue_entries(v, p, v->d_pos, v->d_dir, v->d_state, st)) return rc;
    const size_t n = (size_t)v->probes * p->dirs;
    if (pos) HIPCHK(hipMemcpyAsync(pos, v->d_pos, n * 12u, hipMemcpyDeviceToHost, st));
    if (dir) HIPCHK(hipMemcpyAsync(dir, v->d_dir, n * 12u, hipMemcpyDeviceToHost, st));
    if (state) HIPCHK(hipMemcpyAsync(state, v->d_state, n * 4u, hipMemcpyDeviceToHost, st));
    return end_call_host(v);
}

int rt_probe_volume_entries_device(rt_probe_volume* v, const rt_probe_bake_params* p, void* d_pos, void* d_dir, void* d_state, void* stream) {
    if (const int rc = check_bake_params(v, p)) return rc;
    if (!d_pos && !d_dir && !d_state) return fail(RT_ERR_INVALID, "pos, dir and state are all null");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(v, st)) return rc;
    if (const int rc = enqueue_entries(v, p, (float*)d_pos, (float*)d_dir, (uint32_t*)d_state, st)) return rc;
    return end_call(v, st);
}

int rt_probe_volume_bake(rt_probe_volume* v, const rt_probe_bake_params* p, float* out_sh, rt_probe_stats* stats) {
    if (const int rc = check_bake_params(v, p)) return rc;
    hipStream_t st = v->stream;
    if (const int rc = bake_enqueue(v, p, nullptr, nullptr, st)) return rc;
    if (out_sh) HIPCHK(hipMemcpyAsync(out_sh, v->d_sh, (size_t)v->probes * 144u, hipMemcpyDeviceToHost, st));
    if (stats) HIPCHK(hipMemcpyAsync(stats, v->d_stats, sizeof(rt_probe_stats), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_probe_volume_bake_device(rt_probe_volume* v, const rt_probe_bake_params* p, void* d_out_sh, void* d_stats, void* stream) {
    if (const int rc = check_bake_params(v, p)) return rc;
    return bake_enqueue(v, p, (float4*)d_out_sh, (rt_probe_stats*)d_stats, (hipStream_t)stream);
}

int rt_probe_volume_set_sh(rt_probe_volume* v, const float* sh) {
    if (!v || !sh) return fail(RT_ERR_INVALID, "null argument");
    hipStream_t st = v->stream;
    if (const int rc = begin_call(v, st)) return rc;
    HIPCHK(hipMemcpyAsync(v->d_sh, sh, (size_t)v->probes * 144u, hipMemcpyHostToDevice, st));
    v->has_table = true;
    return end_call_host(v);
}

int rt_probe_volume_set_sh_device(rt_probe_volume* v, const void* d_sh, void* stream) {
    if (!v || !d_sh) return fail(RT_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(v, st)) return rc;
    HIPCHK(hipMemcpyAsync(v->d_sh, d_sh, (size_t)v->probes * 144u, hipMemcpyDeviceToDevice, st));
    v->has_table = true;
    return end_call(v, st);
}

int rt_probe_volume_get_sh(rt_probe_volume* v, float* sh) {
    if (!v || !sh) return fail(RT_ERR_INVALID, "null argument");
    if (!v->has_table) return fail(RT_ERR_INVALID, "the volume holds no table yet: get_sh needs a bake or a set_sh first");
    hipStream_t st = v->stream;
    if (const int rc = begin_call(v, st)) return rc;
    HIPCHK(hipMemcpyAsync(sh, v->d_sh, (size_t)v->probes * 144u, hipMemcpyDeviceToHost, st));
    return end_call_host(v);
}

int rt_probe_volume_get_sh_device(rt_probe_volume* v, void* d_sh, void* stream) {
    if (!v || !d_sh) return fail(RT_ERR_INVALID, "null argument");
    if (!v->has_table) return fail(RT_ERR_INVALID, "the volume holds no table yet: get_sh needs a bake or a set_sh first");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(v, st)) return rc;
    HIPCHK(hipMemcpyAsync(d_sh, v->d_sh, (size_t)v->probes * 144u, hipMemcpyDeviceToDevice, st));
    return end_call(v, st);
}

int rt_probe_volume_sample(rt_probe_volume* v, uint32_t n, const float* pos, const float* normal, float* out_rgb) {
    if (const int rc = sample_check(v, n, pos, normal, out_rgb)) return rc;
    if (n == 0) return RT_OK;
    hipStream_t st = v->stream;
    if (const int rc = begin_call(v, st)) return rc;
    float* d_pos = v->d_host_pts;
    float* d_nrm = d_pos + 3 * (size_t)kPvStagePoints;
    float* d_out = d_nrm + 3 * (size_t)kPvStagePoints;
    for (uint32_t i0 = 0; i0 < n; i0 += kPvStagePoints) { // the staging is the volume's, allocated at creation: a piece at a time, in stream order
        const uint32_t m = n - i0 < kPvStagePoints ? n - i0 : kPvStagePoints;
        HIPCHK(hipMemcpyAsync(d_pos, pos + 3 * (size_t)i0, (size_t)m * 12u, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_nrm, normal + 3 * (size_t)i0, (size_t)m * 12u, hipMemcpyHostToDevice, st));
        if (const int rc = enqueue_sample(v, m, d_pos, d_nrm, d_out, st)) return rc;
        HIPCHK(hipMemcpyAsync(out_rgb + 3 * (size_t)i0, d_out, (size_t)m * 12u, hipMemcpyDeviceToHost, st));
    }
    return end_call_host(v);
}

int rt_probe_volume_sample_device(rt_probe_volume* v, uint32_t n, const void* d_pos, const void* d_normal, void* d_out_rgb, void* stream) {
    if (const int rc = sample_check(v, n, d_pos, d_normal, d_out_rgb)) return rc;
    if (n == 0) return RT_OK;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(v, st)) return rc;
    if (const int rc = enqueue_sample(v, n, (const float*)d_pos, (const float*)d_normal, (float*)d_out_rgb, st)) return rc;
    return end_call(v, st);
}

} // extern "C"
