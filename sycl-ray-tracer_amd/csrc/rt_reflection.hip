// rt_reflection.hip — reflection probes: rt_reflection_probes_create / _destroy, rt_reflection_probes_entries[_device], _bake[_device],
// _set_level0[_device], _prefilter[_device], _get_chain[_device], _sample[_device], and their kernels. A set of cube-map captures over one
// scene, each with a chain of levels prefiltered for growing roughness, for glossy light along a reflection vector where nothing is
// parametrised (moving objects, particles, a rasterised pass). The bake is a composition around one path query (rt_path_query.hip, called
// through its public entry point), as the probe volume's is: the cube faces' jittered rays and a state each (k_rf_entries), the mean per
// texel (k_rf_resolve), the cosine-power prefilter of every higher level from level 0 (k_rf_prefilter), and apart from the bake the cube
// lookup with parallax correction and level interpolation at caller-supplied points (k_rf_sample). The arithmetic is the contract stated at
// rt_reflection_probes_bake in include/rt_mi355x.h; the numpy model that pins it bit for bit is tests/test_reflection_probe.py. No
// traversal, no transcendental function and no float atomics in this unit: a prefiltered texel is one lane's sequential sum over the
// level-0 texels in layout order (LDS only hands every lane the same source), the statistics are ballots and integer sums.
#include "rt_internal.h"
#include "rt_device.h"

struct rt_reflection_probes : CallBracket { // the host forms run on its stream
    rt_scene* scene = nullptr;
    uint32_t count = 0, size = 0, levels = 0, max_spt = 0;
    uint32_t face0 = 0;              // 6 * size * size: the texels of one probe's level 0, the length of a prefilter sum
    uint32_t chain = 0;              // texels of one probe's chain
    bool has_box = false;
    float* d_centre = nullptr;       // 3 floats per probe
    float* d_box = nullptr;          // 6 floats per probe (has_box)
    float4* d_table = nullptr;       // face0 float4: (d_k, o_k)
    float* d_pos = nullptr;          // 3 floats per entry (count * face0 * max_spt entries)
    float* d_dir = nullptr;          // 3 floats per entry
    uint32_t* d_state = nullptr;     // per entry
    float* d_rad = nullptr;          // 3 floats per entry
    uint32_t* d_rays = nullptr;      // per entry
    float4* d_chain = nullptr;       // count * chain float4
    rt_reflection_stats* d_stats = nullptr;
    uint8_t* d_host_pts = nullptr;   // the host form of sample: kRfStagePoints points at a time, index | pos | dir | lod | rgb
    bool has_level0 = false;         // a bake or a set_level0 was enqueued
    bool levels_fresh = false;       // the levels above 0 were made from the level 0 held
};

namespace rt {

constexpr uint32_t kRfBlock = 256;      // every kernel of this unit
constexpr uint32_t kRfWaves = kRfBlock / 64u;
#ifndef RT_RF_SAMPLE_WAVES
#define RT_RF_SAMPLE_WAVES 8
#endif
#ifndef RT_RF_PIECE
#define RT_RF_PIECE 1024
#endif
constexpr uint32_t kRfPiece = RT_RF_PIECE; // level-0 texels k_rf_prefilter stages at a time, 32 bytes each (DESIGN.md §23 has the other source path)
constexpr uint32_t kRfSampleWaves = RT_RF_SAMPLE_WAVES; // waves per SIMD k_rf_sample's register budget allows

// what the kernels read of a probe set
struct RfShape {
    uint32_t count, size, levels;
    uint32_t face0, chain; // texels of a probe's level 0 and of its whole chain
};

RT_DEV uint32_t rf_level_offset(uint32_t size, uint32_t l) { // texels of a probe's chain in front of level l
    uint32_t o = 0;
    for (uint32_t m = 0; m < l; ++m) o += 6u * (size >> m) * (size >> m);
    return o;
}

// the cube: face f at (s, t) in [-1, 1]^2, unnormalised (the table in include/rt_mi355x.h)
RT_DEV f3 rf_face_dir(uint32_t f, float s, float t) {
    switch (f) {
    case 0: return mk3(1.0f, -t, -s);
    case 1: return mk3(-1.0f, -t, s);
    case 2: return mk3(s, 1.0f, t);
    case 3: return mk3(s, -1.0f, -t);
    case 4: return mk3(s, -t, 1.0f);
    default: return mk3(-s, -t, -1.0f);
    }
}
RT_DEV float rf_centre(uint32_t x, uint32_t S) { return __fsub_rn(__fmul_rn(__fadd_rn((float)x, 0.5f), 2.0f / (float)S), 1.0f); }
// v * i and i = 1 / sqrt(dot(v, v)), R2's normalize; .w = (i * i) * i
RT_DEV float4 rf_unit_and_weight(f3 v) {
    const float i = 1.0f / __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y)), __fmul_rn(v.z, v.z)));
    return make_float4(__fmul_rn(v.x, i), __fmul_rn(v.y, i), __fmul_rn(v.z, i), __fmul_rn(__fmul_rn(i, i), i));
}

// The table of step 4, one thread per level-0 texel k of a probe: its unit centre direction and its solid-angle weight
__global__ void __launch_bounds__(kRfBlock) k_rf_table(uint32_t size, float4* __restrict__ table) {
    const uint32_t k = blockIdx.x * kRfBlock + threadIdx.x;
    if (k >= 6u * size * size) return;
    const uint32_t x = k % size, y = (k / size) % size, f = k / (size * size);
    table[k] = rf_unit_and_weight(rf_face_dir(f, rf_centre(x, size), rf_centre(y, size)));
}

// Step 1, one thread per entry e = T * spt + j: the probe's position, the jittered face direction and the state its two draws leave.
// NULL outputs are not written.
__global__ void __launch_bounds__(kRfBlock) k_rf_entries(RfShape G, const float* __restrict__ centre, uint32_t n, uint32_t spt, uint32_t seed,
                                                          float* __restrict__ pos_out, float* __restrict__ dir_out, uint32_t* __restrict__ state_out) {
    const uint32_t e = blockIdx.x * kRfBlock + threadIdx.x; // below 2^31 (rt_reflection_probes_create)
    if (e >= n) return;
    const uint32_t T = e / spt;
    const uint32_t x = T % G.size, y = (T / G.size) % G.size, f = (T / (G.size * G.size)) % 6u, p = T / G.face0;
    uint32_t a = seed + (e + 1u) * 0x9E3779B9u;
    a = a ? a : 0x9E3779B9u;
    const float u1 = rng_next(a), u2 = rng_next(a);
    const float step = 2.0f / (float)G.size;
    const float s = __fsub_rn(__fmul_rn(__fadd_rn((float)x, u1), step), 1.0f);
    const float t = __fsub_rn(__fmul_rn(__fadd_rn((float)y, u2), step), 1.0f);
    if (pos_out) {
        pos_out[3 * (size_t)e] = centre[3 * p], pos_out[3 * (size_t)e + 1] = centre[3 * p + 1], pos_out[3 * (size_t)e + 2] = centre[3 * p + 2];
    }
    if (dir_out) {
        const f3 d = rf_face_dir(f, s, t);
        dir_out[3 * (size_t)e] = d.x, dir_out[3 * (size_t)e + 1] = d.y, dir_out[3 * (size_t)e + 2] = d.z;
    }
    if (state_out) state_out[e] = a;
}

// Steps 3 and 5, one thread per level-0 texel T: the mean of its spt entries into the probe's chain. A probe is valid iff its entries were not
// rejected (the path query rejects an entry by its origin, which a probe's entries share). The statistics: valid probes as a ballot of their
// first texels' lanes, their entries' rays as a wave sum; lane 0 of every wave adds them.
__global__ void __launch_bounds__(kRfBlock) k_rf_resolve(RfShape G, const float* __restrict__ rad, const uint32_t* __restrict__ rays, uint32_t spt,
                                                          float clamp, float4* __restrict__ chain, rt_reflection_stats* __restrict__ stats) {
    const uint32_t T = blockIdx.x * kRfBlock + threadIdx.x; // below 2^31
    bool counted = false;
    unsigned long long traced = 0;
    if (T < G.count * G.face0) {
        const uint32_t p = T / G.face0, k = T % G.face0;
        const size_t e0 = (size_t)T * spt;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (rays[e0] != 0xFFFFFFFFu) {
            float cx = 0.0f, cy = 0.0f, cz = 0.0f;
            for (uint32_t j = 0; j < spt; ++j) {
                const float* r = rad + 3 * (e0 + j);
                float rx = r[0], ry = r[1], rz = r[2];
                if (clamp > 0.0f) rx = __builtin_fminf(rx, clamp), ry = __builtin_fminf(ry, clamp), rz = __builtin_fminf(rz, clamp);
                cx = __fadd_rn(cx, rx), cy = __fadd_rn(cy, ry), cz = __fadd_rn(cz, rz);
                traced += rays[e0 + j];
            }
            const float d = (float)spt;
            o = make_float4(cx / d, cy / d, cz / d, 1.0f);
            counted = k == 0u;
        }
        chain[(size_t)p * G.chain + k] = o;
    }
    const uint32_t n_valid = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(counted));
    for (int off = 32; off > 0; off >>= 1) traced += __shfl_xor(traced, off, 64);
    if ((threadIdx.x & 63u) == 0u) {
        if (T == 0u) stats->probes = G.count; // the other two words were zeroed on the stream and are only added to
        if (n_valid) atomicAdd(&stats->valid, n_valid);
        if (traced) atomicAdd((unsigned long long*)&stats->rays, traced);
    }
}

// Step 4, the terms of one staged piece for one output direction n, the lobe cos^(2^Q): every lane of every wave walks the same m terms in
// the same order, so each read of the piece has one address for the whole wave and is a broadcast. A term that is not in front is left out
// by selects: its weight multiplies nothing.
template <int Q>
RT_DEV void rf_lobe_piece(const float4* stage, uint32_t m, f3 n, float& W, float& ax, float& ay, float& az) {
#pragma unroll 4 // the reads of four terms in flight; the sums stay in order
    for (uint32_t k = 0; k < m; ++k) {
        const float4 d = stage[2u * k], r = stage[2u * k + 1u];
        const float c = __fadd_rn(__fadd_rn(__fmul_rn(n.x, d.x), __fmul_rn(n.y, d.y)), __fmul_rn(n.z, d.z));
        float w = c;
#pragma unroll
        for (int j = 0; j < Q; ++j) w = __fmul_rn(w, w);
        w = __fmul_rn(w, d.w);
        const bool on = c > 0.0f;
        const float W1 = __fadd_rn(W, w), x1 = __fadd_rn(ax, __fmul_rn(w, r.x)), y1 = __fadd_rn(ay, __fmul_rn(w, r.y)), z1 = __fadd_rn(az, __fmul_rn(w, r.z));
        W = on ? W1 : W, ax = on ? x1 : ax, ay = on ? y1 : ay, az = on ? z1 : az;
    }
}

// Step 4. A wave is one unit of work: 64 consecutive outputs of one level of one probe (the last unit of a level may be part full: 96
// outputs are 64 + 32). A probe's units, level 1 first, are dealt to workgroups of kRfWaves waves, and the workgroups of all probes form one
// grid, so the few outputs of the small levels of many probes fill the device together. The workgroup's waves share the probe and with it
// the source: kRfPiece terms at a time, (d_k, o_k) and the texel interleaved, staged through LDS by all of its lanes (the idle waves of
// a probe's last workgroup included) and read back with identical addresses. The level and with it the number of squarings are the wave's
// (readfirstlane makes the wave index scalar); the barriers stand outside that choice.
__global__ void __launch_bounds__(kRfBlock) k_rf_prefilter(RfShape G, uint32_t units, uint32_t groups, const float4* __restrict__ table,
                                                            const float4* __restrict__ level0, float4* __restrict__ out) {
    __shared__ float4 stage[2u * kRfPiece];
    const uint32_t p = blockIdx.x / groups; // below count: the grid is count * groups
    uint32_t u = (blockIdx.x % groups) * kRfWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t l = 1, S = G.size >> 1, off = G.face0;
    bool active = u < units;
    if (active)
        for (;;) { // levels >= 2 here, and u < units: the walk ends inside the chain
            const uint32_t lu = (6u * S * S + 63u) >> 6;
            if (u < lu) break;
            u -= lu, off += 6u * S * S, ++l, S >>= 1;
        }
    const uint32_t o = u * 64u + (threadIdx.x & 63u);
    active = active && o < 6u * S * S;
    const float4* src = level0 + (size_t)p * G.chain;
    const bool valid = src[0].w != 0.0f; // the workgroup's
    f3 n = mk3(0.0f, 0.0f, 0.0f);
    if (active) {
        const uint32_t x = o % S, y = (o / S) % S, f = o / (S * S);
        const float4 nn = rf_unit_and_weight(rf_face_dir(f, rf_centre(x, S), rf_centre(y, S)));
        n = mk3(nn.x, nn.y, nn.z);
    }
    float W = 0.0f, ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (valid)
        for (uint32_t base = 0; base < G.face0; base += kRfPiece) {
            const uint32_t m = G.face0 - base < kRfPiece ? G.face0 - base : kRfPiece;
            __syncthreads(); // the piece before this one has been read
            for (uint32_t i = threadIdx.x; i < m; i += kRfBlock) stage[2u * i] = table[base + i], stage[2u * i + 1u] = src[base + i];
            __syncthreads();
            if (active) switch (G.levels - l) { // q = 2 * (levels - l) - 1 squarings
                case 1: rf_lobe_piece<1>(stage, m, n, W, ax, ay, az); break;
                case 2: rf_lobe_piece<3>(stage, m, n, W, ax, ay, az); break;
                case 3: rf_lobe_piece<5>(stage, m, n, W, ax, ay, az); break;
                case 4: rf_lobe_piece<7>(stage, m, n, W, ax, ay, az); break;
                default: rf_lobe_piece<9>(stage, m, n, W, ax, ay, az); break;
                }
        }
    if (active) out[(size_t)p * G.chain + off + o] = valid ? make_float4(ax / W, ay / W, az / W, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}


// One level of step 6: the four taps about (s, t) on face f of level l, y outer
RT_DEV f3 rf_bilinear(const float4* __restrict__ lvl, uint32_t S, uint32_t f, float s, float t) {
    const float half = __fmul_rn(0.5f, (float)S), top = (float)(S - 1u);
    const float fx = __builtin_fminf(__builtin_fmaxf(__fsub_rn(__fmul_rn(__fadd_rn(s, 1.0f), half), 0.5f), 0.0f), top);
    const float fy = __builtin_fminf(__builtin_fmaxf(__fsub_rn(__fmul_rn(__fadd_rn(t, 1.0f), half), 0.5f), 0.0f), top);
    const int32_t ix = (int32_t)fx, iy = (int32_t)fy, lim = (int32_t)S - 2; // S >= 4
    const uint32_t x0 = (uint32_t)(ix < lim ? ix : lim), y0 = (uint32_t)(iy < lim ? iy : lim);
    const float gx = __fsub_rn(fx, (float)x0), gy = __fsub_rn(fy, (float)y0);
    const float wx[2] = {__fsub_rn(1.0f, gx), gx}, wy[2] = {__fsub_rn(1.0f, gy), gy};
    const float4* base = lvl + ((size_t)f * S + y0) * S + x0; // the four taps lie inside the face: x0 + 1, y0 + 1 <= S - 1
    const float4 v[4] = {base[0], base[1], base[S], base[S + 1u]};
    f3 a = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float w = __fmul_rn(wy[k >> 1], wx[k & 1]);
        a.x = __fadd_rn(a.x, __fmul_rn(w, v[k].x)), a.y = __fadd_rn(a.y, __fmul_rn(w, v[k].y)), a.z = __fadd_rn(a.z, __fmul_rn(w, v[k].z));
    }
    return a;
}

// Step 6, one thread per point: at most 8 float4 loads of the chain beside the probe's validity
__global__ void __launch_bounds__(kRfBlock, kRfSampleWaves) k_rf_sample(RfShape G, const float4* __restrict__ chain, const float* __restrict__ centre,
                                                                        const float* __restrict__ box, uint32_t n, const uint32_t* __restrict__ index,
                                                                        const float* __restrict__ pos, const float* __restrict__ dir,
                                                                        const float* __restrict__ lod, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kRfBlock + threadIdx.x;
    if (i >= n) return;
    float* o = out + 3 * (size_t)i;
    const uint32_t p = index[i];
    f3 r = mk3(dir[3 * (size_t)i], dir[3 * (size_t)i + 1], dir[3 * (size_t)i + 2]);
    float ld = lod[i];
    bool ok = p < G.count && __builtin_isfinite(r.x) && __builtin_isfinite(r.y) && __builtin_isfinite(r.z) && __builtin_isfinite(ld);
    f3 q = mk3(0.0f, 0.0f, 0.0f);
    if (pos) {
        q = mk3(pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]);
        ok = ok && __builtin_isfinite(q.x) && __builtin_isfinite(q.y) && __builtin_isfinite(q.z);
    }
    if (ok && pos && box) { // the parallax box
        const float* b = box + 6 * (size_t)p;
        const float inf = __uint_as_float(0x7F800000u);
        const float tx = r.x == 0.0f ? inf : __fsub_rn(r.x > 0.0f ? b[3] : b[0], q.x) / r.x;
        const float ty = r.y == 0.0f ? inf : __fsub_rn(r.y > 0.0f ? b[4] : b[1], q.y) / r.y;
        const float tz = r.z == 0.0f ? inf : __fsub_rn(r.z > 0.0f ? b[5] : b[2], q.z) / r.z;
        const float t = __builtin_fminf(__builtin_fminf(tx, ty), tz);
        if (t > 0.0f && __builtin_isfinite(t)) {
            const float* c = centre + 3 * (size_t)p;
            r = mk3(__fsub_rn(__fadd_rn(q.x, __fmul_rn(r.x, t)), c[0]), __fsub_rn(__fadd_rn(q.y, __fmul_rn(r.y, t)), c[1]),
                    __fsub_rn(__fadd_rn(q.z, __fmul_rn(r.z, t)), c[2]));
            ok = __builtin_isfinite(r.x) && __builtin_isfinite(r.y) && __builtin_isfinite(r.z);
        }
    }
    const float mx = __builtin_fabsf(r.x), my = __builtin_fabsf(r.y), mz = __builtin_fabsf(r.z);
    const uint32_t axis = (mx >= my && mx >= mz) ? 0u : (my >= mz ? 1u : 2u);
    const float m = axis == 0u ? mx : (axis == 1u ? my : mz);
    if (!ok || !(m > 0.0f)) {
        o[0] = o[1] = o[2] = __uint_as_float(0x7FC00000u);
        return;
    }
    const float4* c = chain + (size_t)p * G.chain;
    if (c[0].w == 0.0f) { // an invalid probe
        o[0] = o[1] = o[2] = 0.0f;
        return;
    }
    uint32_t f;
    float s, t;
    if (axis == 0u) f = r.x > 0.0f ? 0u : 1u, s = (r.x > 0.0f ? -r.z : r.z) / m, t = -r.y / m;
    else if (axis == 1u) f = r.y > 0.0f ? 2u : 3u, s = r.x / m, t = (r.y > 0.0f ? r.z : -r.z) / m;
    else f = r.z > 0.0f ? 4u : 5u, s = (r.z > 0.0f ? r.x : -r.x) / m, t = -r.y / m;
    ld = __builtin_fminf(__builtin_fmaxf(ld, 0.0f), (float)(G.levels - 1u));
    if (G.levels == 1u) {
        const f3 a = rf_bilinear(c, G.size, f, s, t);
        o[0] = a.x, o[1] = a.y, o[2] = a.z;
        return;
    }
    const int32_t il = (int32_t)ld, ltop = (int32_t)G.levels - 2;
    const uint32_t l0 = (uint32_t)(il < ltop ? il : ltop);
    const float fl = __fsub_rn(ld, (float)l0), f0 = __fsub_rn(1.0f, fl);
    const uint32_t off0 = rf_level_offset(G.size, l0), S0 = G.size >> l0;
    const f3 a = rf_bilinear(c + off0, S0, f, s, t);
    const f3 b = rf_bilinear(c + off0 + 6u * S0 * S0, S0 >> 1, f, s, t);
    o[0] = __fadd_rn(__fmul_rn(a.x, f0), __fmul_rn(b.x, fl));
    o[1] = __fadd_rn(__fmul_rn(a.y, f0), __fmul_rn(b.y, fl));
    o[2] = __fadd_rn(__fmul_rn(a.z, f0), __fmul_rn(b.z, fl));
}

} // namespace rt

namespace {

static_assert(sizeof(rt_reflection_probes_desc) == 32 && sizeof(rt_reflection_bake_params) == 20 && sizeof(rt_reflection_stats) == 16,
              "include/rt_mi355x.h states the sizes");

constexpr uint32_t kMaxCount = 4096, kMinSize = 8, kMaxSize = 128, kMaxSpt = 1024;
constexpr uint32_t kRfStagePoints = 65536; // points the host form of sample stages at a time: 44 bytes each

RfShape shape_of(const rt_reflection_probes* r) { return RfShape{r->count, r->size, r->levels, r->face0, r->chain}; }
size_t chain_bytes(const rt_reflection_probes* r) { return (size_t)r->count * r->chain * 16u; }
size_t level0_bytes(const rt_reflection_probes* r) { return (size_t)r->face0 * 16u; } // of one probe

int check_bake_params(const rt_reflection_probes* r, const rt_reflection_bake_params* p) {
    if (!r || !p) return fail(RT_ERR_INVALID, "null argument");
    if (p->spt == 0) return fail(RT_ERR_INVALID, "spt must be at least 1");
    if (p->spt > r->max_spt) return fail(RT_ERR_INVALID, "spt exceeds the max_spt the probes were created with");
    if (p->max_depth == 0) return fail(RT_ERR_INVALID, "max_depth must be at least 1");
    if (!(p->clamp >= 0.0f)) return fail(RT_ERR_INVALID, "clamp must be 0 (off) or above, not NaN");
    return RT_OK;
}

int check_held(const rt_reflection_probes* r, const char* what) {
    if (!r->has_level0) return fail(RT_ERR_INVALID, std::string("the probes hold no level 0 yet: ") + what + " needs a bake or a set_level0 first");
    return RT_OK;
}

// the end of a host form whose copies lie inside the bracket: the call's end, then the stream has run dry
int end_call_host(rt_reflection_probes* r) {
    if (const int rc = end_call(r, r->stream)) return rc;
    HIPCHK(hipStreamSynchronize(r->stream));
    return RT_OK;
}

// step 1 on st into device pointers, any of them null. PRE: the call's bracket is open
int enqueue_entries(rt_reflection_probes* r, const rt_reflection_bake_params* p, float* pos, float* dir, uint32_t* state, hipStream_t st) {
    const uint32_t n = r->count * r->face0 * p->spt;
    hipLaunchKernelGGL(k_rf_entries, dim3((n + kRfBlock - 1u) / kRfBlock), dim3(kRfBlock), 0, st, shape_of(r), (const float*)r->d_centre, n, p->spt,
                       p->seed, pos, dir, state);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// step 4 on st, from the level 0 the chain holds. PRE: the call's bracket is open
int enqueue_prefilter(rt_reflection_probes* r, hipStream_t st) {
    r->levels_fresh = true;
    if (r->levels == 1) return RT_OK;
    uint32_t units = 0;
    for (uint32_t l = 1; l < r->levels; ++l) units += (6u * (r->size >> l) * (r->size >> l) + 63u) / 64u;
    const uint32_t groups = (units + kRfWaves - 1u) / kRfWaves;
    hipLaunchKernelGGL(k_rf_prefilter, dim3(r->count * groups), dim3(kRfBlock), 0, st, shape_of(r), units, groups, (const float4*)r->d_table,
                       (const float4*)r->d_chain, r->d_chain);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// rt_reflection_probes_bake[_device]: steps 1 to 5 on st; the chain stays in d_chain. out / stats: device pointers or null. PRE: the arguments were checked
int bake_enqueue(rt_reflection_probes* r, const rt_reflection_bake_params* p, float4* out, rt_reflection_stats* stats, hipStream_t st) {
    if (const int rc = begin_call(r, st)) return rc;
    if (const int rc = enqueue_entries(r, p, r->d_pos, r->d_dir, r->d_state, st)) return rc;
    rt_path_query q{};
    q.n = r->count * r->face0 * p->spt, q.max_depth = p->max_depth, q.samples = 1, q.rr_start = p->rr_start;
    q.org = r->d_pos, q.dir = r->d_dir, q.rng = r->d_state, q.rng_out = nullptr, q.radiance = r->d_rad, q.rays = r->d_rays;
    if (const int rc = rt_trace_paths_device(r->scene, &q, st)) return rc; // records the scene's event for st
    HIPCHK(hipSetDevice(r->device));
    rt_reflection_stats* d_stats = stats ? stats : r->d_stats;
    HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(rt_reflection_stats), st));
    const uint32_t texels = r->count * r->face0;
    hipLaunchKernelGGL(k_rf_resolve, dim3((texels + kRfBlock - 1u) / kRfBlock), dim3(kRfBlock), 0, st, shape_of(r), (const float*)r->d_rad,
                       (const uint32_t*)r->d_rays, p->spt, p->clamp, r->d_chain, d_stats);
    HIPCHK(hipGetLastError());
    r->has_level0 = true;
    if (const int rc = enqueue_prefilter(r, st)) return rc;
    if (out) HIPCHK(hipMemcpyAsync(out, r->d_chain, chain_bytes(r), hipMemcpyDeviceToDevice, st));
    return end_call(r, st);
}

// level 0 of every probe from `src` (count * face0 float4, probes consecutive) into the chain. PRE: the call's bracket is open
int enqueue_set_level0(rt_reflection_probes* r, const void* src, hipMemcpyKind kind, hipStream_t st) {
    HIPCHK(hipMemcpy2DAsync(r->d_chain, (size_t)r->chain * 16u, src, level0_bytes(r), level0_bytes(r), r->count, kind, st));
    r->has_level0 = true, r->levels_fresh = r->levels == 1;
    return RT_OK;
}

int sample_check(const rt_reflection_probes* r, uint32_t n, const void* index, const void* dir, const void* lod, const void* out) {
    if (!r) return fail(RT_ERR_INVALID, "null argument");
    if (n && (!index || !dir || !lod || !out)) return fail(RT_ERR_INVALID, "null probe_index, dir, lod or output");
    if (const int rc = check_held(r, "sample")) return rc;
    if (!r->levels_fresh) return fail(RT_ERR_INVALID, "the levels above 0 are stale after set_level0: sample needs a prefilter first");
    return RT_OK;
}

// k_rf_sample over n device points on st. PRE: the call's bracket is open, n > 0
int enqueue_sample(rt_reflection_probes* r, uint32_t n, const uint32_t* index, const float* pos, const float* dir, const float* lod, float* out,
                   hipStream_t st) {
    hipLaunchKernelGGL(k_rf_sample, dim3((n + kRfBlock - 1u) / kRfBlock), dim3(kRfBlock), 0, st, shape_of(r), (const float4*)r->d_chain,
                       (const float*)r->d_centre, (const float*)(r->has_box ? r->d_box : nullptr), n, index, pos, dir, lod, out);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

} // namespace

extern "C" {

int rt_reflection_probes_create(rt_scene* s, const rt_reflection_probes_desc* d, uint32_t flags, rt_reflection_probes** out) {
    if (!out) return fail(RT_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (!s) return fail(RT_ERR_INVALID, "null scene");
    if (!d) return fail(RT_ERR_INVALID, "null description");
    if (!d->pos) return fail(RT_ERR_INVALID, "null positions");
    if (d->count < 1 || d->count > kMaxCount) return fail(RT_ERR_INVALID, "count must be 1 .. 4096");
    if (d->size < kMinSize || d->size > kMaxSize || (d->size & (d->size - 1u))) return fail(RT_ERR_INVALID, "size must be a power of two in 8 .. 128");
    uint32_t log2 = 0;
    while ((1u << log2) < d->size) ++log2;
    if (d->levels < 1 || d->levels > log2 - 1u) return fail(RT_ERR_INVALID, "levels must be 1 .. log2(size) - 1 (the smallest face is 4)");
    if (d->max_spt < 1 || d->max_spt > kMaxSpt) return fail(RT_ERR_INVALID, "max_spt must be 1 .. 1024");
    const uint64_t face0 = 6ull * d->size * d->size;
    if ((uint64_t)d->count * face0 * d->max_spt > 0x7fffffffull)
        return fail(RT_ERR_INVALID, "too many entries (count x 6 x size^2 x max_spt must stay below 2^31)");
    for (uint32_t i = 0; i < 3u * d->count; ++i)
        if (!std::isfinite(d->pos[i])) return fail(RT_ERR_INVALID, "every position must be finite");
    if (d->box)
        for (uint32_t p = 0; p < d->count; ++p) {
            const float* b = d->box + 6 * (size_t)p;
            for (int a = 0; a < 6; ++a)
                if (!std::isfinite(b[a])) return fail(RT_ERR_INVALID, "every box value must be finite");
            for (int a = 0; a < 3; ++a)
                if (b[a] > b[3 + a]) return fail(RT_ERR_INVALID, "a box has min above max");
        }
    if (flags) return fail(RT_ERR_INVALID, "unknown reflection probe flag");
    if (s->device < 0) return fail(RT_ERR_NO_DEVICE, "scene was built host-only (device < 0)");
    HIPCHK(hipSetDevice(s->device));
    return no_throw([&]() -> int {
        rt_reflection_probes* r = new rt_reflection_probes;
        r->scene = s, r->device = s->device, r->count = d->count, r->size = d->size, r->levels = d->levels, r->max_spt = d->max_spt;
        r->face0 = (uint32_t)face0, r->has_box = d->box != nullptr;
        for (uint32_t l = 0; l < d->levels; ++l) r->chain += 6u * (d->size >> l) * (d->size >> l);
        const size_t e = (size_t)d->count * face0 * d->max_spt;
        if (hipMalloc((void**)&r->d_centre, (size_t)d->count * 12u) != hipSuccess || hipMalloc((void**)&r->d_box, (size_t)d->count * 24u) != hipSuccess ||
            hipMalloc((void**)&r->d_table, (size_t)face0 * 16u) != hipSuccess || hipMalloc((void**)&r->d_pos, e * 12u) != hipSuccess ||
            hipMalloc((void**)&r->d_dir, e * 12u) != hipSuccess || hipMalloc((void**)&r->d_state, e * 4u) != hipSuccess ||
            hipMalloc((void**)&r->d_rad, e * 12u) != hipSuccess || hipMalloc((void**)&r->d_rays, e * 4u) != hipSuccess ||
            hipMalloc((void**)&r->d_chain, chain_bytes(r)) != hipSuccess || hipMalloc((void**)&r->d_stats, sizeof(rt_reflection_stats)) != hipSuccess ||
            hipMalloc((void**)&r->d_host_pts, (size_t)kRfStagePoints * 44u) != hipSuccess) {
            rt_reflection_probes_destroy(r);
            return fail(RT_ERR_OOM, "hipMalloc of the reflection probes' buffers failed");
        }
        int rc = bracket_open(r);
        if (!rc) { // the copies of the description and the table, on the object's stream; creation returns when they are done
            const hipError_t e0 = hipMemcpyAsync(r->d_centre, d->pos, (size_t)d->count * 12u, hipMemcpyHostToDevice, r->stream);
            const hipError_t e1 = d->box ? hipMemcpyAsync(r->d_box, d->box, (size_t)d->count * 24u, hipMemcpyHostToDevice, r->stream) : hipSuccess;
            hipLaunchKernelGGL(k_rf_table, dim3((r->face0 + kRfBlock - 1u) / kRfBlock), dim3(kRfBlock), 0, r->stream, r->size, r->d_table);
            if (e0 != hipSuccess || e1 != hipSuccess || hipGetLastError() != hipSuccess || hipStreamSynchronize(r->stream) != hipSuccess)
                rc = fail(RT_ERR_HIP, "the copies or the table kernel of the reflection probes' creation failed");
        }
        if (rc) {
            rt_reflection_probes_destroy(r);
            return rc;
        }
        *out = r;
        return (int)RT_OK;
    });
}

void rt_reflection_probes_destroy(rt_reflection_probes* r) {
    if (!r) return;
    if (bracket_close(r))
        for (void* p : {(void*)r->d_centre, (void*)r->d_box, (void*)r->d_table, (void*)r->d_pos, (void*)r->d_dir, (void*)r->d_state, (void*)r->d_rad,
                        (void*)r->d_rays, (void*)r->d_chain, (void*)r->d_stats, (void*)r->d_host_pts})
            (void)hipFree(p);
    delete r;
}

int rt_reflection_probes_entries(rt_reflection_probes* r, const rt_reflection_bake_params* p, float* pos, float* dir, uint32_t* state) {
    if (const int rc = check_bake_params(r, p)) return rc;
    if (!pos && !dir && !state) return fail(RT_ERR_INVALID, "pos, dir and state are all null");
    hipStream_t st = r->stream;
    if (const int rc = begin_call(r, st)) return rc;
    if (const int rc = enqueue_entries(r, p, r->d_pos, r->d_dir, r->d_state, st)) return rc;
    const size_t n = (size_t)r->count * r->face0 * p->spt;
    if (pos) HIPCHK(hipMemcpyAsync(pos, r->d_pos, n * 12u, hipMemcpyDeviceToHost, st));
    if (dir) HIPCHK(hipMemcpyAsync(dir, r->d_dir, n * 12u, hipMemcpyDeviceToHost, st));
    if (state) HIPCHK(hipMemcpyAsync(state, r->d_state, n * 4u, hipMemcpyDeviceToHost, st));
    return end_call_host(r);
}

int rt_reflection_probes_entries_device(rt_reflection_probes* r, const rt_reflection_bake_params* p, void* d_pos, void* d_dir, void* d_state,
                                        void* stream) {
    if (const int rc = check_bake_params(r, p)) return rc;
    if (!d_pos && !d_dir && !d_state) return fail(RT_ERR_INVALID, "pos, dir and state are all null");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(r, st)) return rc;
    if (const int rc = enqueue_entries(r, p, (float*)d_pos, (float*)d_dir, (uint32_t*)d_state, st)) return rc;
    return end_call(r, st);
}

int rt_reflection_probes_bake(rt_reflection_probes* r, const rt_reflection_bake_params* p, float* out_chain, rt_reflection_stats* stats) {
    if (const int rc = check_bake_params(r, p)) return rc;
    hipStream_t st = r->stream;
    if (const int rc = bake_enqueue(r, p, nullptr, nullptr, st)) return rc;
    if (out_chain) HIPCHK(hipMemcpyAsync(out_chain, r->d_chain, chain_bytes(r), hipMemcpyDeviceToHost, st));
    if (stats) HIPCHK(hipMemcpyAsync(stats, r->d_stats, sizeof(rt_reflection_stats), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return RT_OK;
}

int rt_reflection_probes_bake_device(rt_reflection_probes* r, const rt_reflection_bake_params* p, void* d_out_chain, void* d_stats, void* stream) {
    if (const int rc = check_bake_params(r, p)) return rc;
    return bake_enqueue(r, p, (float4*)d_out_chain, (rt_reflection_stats*)d_stats, (hipStream_t)stream);
}

int rt_reflection_probes_set_level0(rt_reflection_probes* r, const float* level0) {
    if (!r || !level0) return fail(RT_ERR_INVALID, "null argument");
    hipStream_t st = r->stream;
    if (const int rc = begin_call(r, st)) return rc;
    if (const int rc = enqueue_set_level0(r, level0, hipMemcpyHostToDevice, st)) return rc;
    return end_call_host(r);
}

int rt_reflection_probes_set_level0_device(rt_reflection_probes* r, const void* d_level0, void* stream) {
    if (!r || !d_level0) return fail(RT_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(r, st)) return rc;
    if (const int rc = enqueue_set_level0(r, d_level0, hipMemcpyDeviceToDevice, st)) return rc;
    return end_call(r, st);
}

int rt_reflection_probes_prefilter(rt_reflection_probes* r) {
    if (!r) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = check_held(r, "prefilter")) return rc;
    hipStream_t st = r->stream;
    if (const int rc = begin_call(r, st)) return rc;
    if (const int rc = enqueue_prefilter(r, st)) return rc;
    return end_call_host(r);
}

int rt_reflection_probes_prefilter_device(rt_reflection_probes* r, void* stream) {
    if (!r) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = check_held(r, "prefilter")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(r, st)) return rc;
    if (const int rc = enqueue_prefilter(r, st)) return rc;
    return end_call(r, st);
}

int rt_reflection_probes_get_chain(rt_reflection_probes* r, float* chain) {
    if (!r || !chain) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = check_held(r, "get_chain")) return rc;
    hipStream_t st = r->stream;
    if (const int rc = begin_call(r, st)) return rc;
    HIPCHK(hipMemcpyAsync(chain, r->d_chain, chain_bytes(r), hipMemcpyDeviceToHost, st));
    return end_call_host(r);
}

int rt_reflection_probes_get_chain_device(rt_reflection_probes* r, void* d_chain, void* stream) {
    if (!r || !d_chain) return fail(RT_ERR_INVALID, "null argument");
    if (const int rc = check_held(r, "get_chain")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(r, st)) return rc;
    HIPCHK(hipMemcpyAsync(d_chain, r->d_chain, chain_bytes(r), hipMemcpyDeviceToDevice, st));
    return end_call(r, st);
}

int rt_reflection_probes_sample(rt_reflection_probes* r, uint32_t n, const uint32_t* probe_index, const float* pos, const float* dir, const float* lod,
                                float* out_rgb) {
    if (const int rc = sample_check(r, n, probe_index, dir, lod, out_rgb)) return rc;
    if (n == 0) return RT_OK;
    hipStream_t st = r->stream;
    if (const int rc = begin_call(r, st)) return rc;
    uint32_t* d_idx = (uint32_t*)r->d_host_pts;
    float* d_pos = (float*)(d_idx + kRfStagePoints);
    float* d_dir = d_pos + 3 * (size_t)kRfStagePoints;
    float* d_lod = d_dir + 3 * (size_t)kRfStagePoints;
    float* d_out = d_lod + kRfStagePoints;
    for (uint32_t i0 = 0; i0 < n; i0 += kRfStagePoints) { // the staging is the object's, allocated at creation: a piece at a time, in stream order
        const uint32_t m = n - i0 < kRfStagePoints ? n - i0 : kRfStagePoints;
        HIPCHK(hipMemcpyAsync(d_idx, probe_index + i0, (size_t)m * 4u, hipMemcpyHostToDevice, st));
        if (pos) HIPCHK(hipMemcpyAsync(d_pos, pos + 3 * (size_t)i0, (size_t)m * 12u, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_dir, dir + 3 * (size_t)i0, (size_t)m * 12u, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_lod, lod + i0, (size_t)m * 4u, hipMemcpyHostToDevice, st));
        if (const int rc = enqueue_sample(r, m, d_idx, pos ? d_pos : nullptr, d_dir, d_lod, d_out, st)) return rc;
        HIPCHK(hipMemcpyAsync(out_rgb + 3 * (size_t)i0, d_out, (size_t)m * 12u, hipMemcpyDeviceToHost, st));
    }
    return end_call_host(r);
}

int rt_reflection_probes_sample_device(rt_reflection_probes* r, uint32_t n, const void* d_probe_index, const void* d_pos, const void* d_dir,
                                       const void* d_lod, void* d_out_rgb, void* stream) {
    if (const int rc = sample_check(r, n, d_probe_index, d_dir, d_lod, d_out_rgb)) return rc;
    if (n == 0) return RT_OK;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = begin_call(r, st)) return rc;
    if (const int rc = enqueue_sample(r, n, (const uint32_t*)d_probe_index, (const float*)d_pos, (const float*)d_dir, (const float*)d_lod,
                                      (float*)d_out_rgb, st))
        return rc;
    return end_call(r, st);
}

} // extern "C"
