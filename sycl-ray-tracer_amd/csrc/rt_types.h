// rt_types.h — data layouts of the device-resident scene and of the kernel parameter block.
// Shared by the host builder (scene_build.cpp, scene_check.cpp) and the HIP kernels (rt_kernels.h, rt_device.h).
#pragma once
#include <cstddef>
#include <cstdint>

namespace rt {

// ---- BVH ----------------------------------------------------------------------------------------
// 4-wide BVH, 64-byte nodes, child boxes quantised to 8 bits per plane on a per-node grid:
//     plane = origin[axis] + q * scale[axis]                  (q = 0..255, scale a power of two)
// quantised conservatively (lo rounded down, hi rounded up) after padding, so a decoded box always
// contains the padded exact box. One node = 4 x dwordx4 loads and decides FOUR children (the first
// version, a BVH2 with fp32 boxes, needed the same 4 loads for two): half the L1 accesses per box
// and half the dependent fetches per ray.
//   word 0-2  origin.xyz (f32)      word 3     scale.x (f32, a power of two: the grid step of the x planes)
//   word 4-9  qlo_x, qhi_x, qlo_y, qhi_y, qlo_z, qhi_z : byte k belongs to child k
//   word 10-11 scale.y, scale.z     word 12-15 child[4]
// (Round 1 packed the three biased exponents into word 3; rebuilding the floats cost 3 x (v_lshlrev 4 + v_and 2 cycles) per
//  node visit on a VALU-bound kernel — profiles/r02_valu_calibration.json — and the two spare words were there.)
// child >= 0: index of an inner node.  child < 0: leaf, ~child = (first << 2) | (count - 1), with
// `first` indexing the leaf-ordered triangle array and 1 <= count <= 4.  child == kChildEmpty: absent.
#ifdef __HIPCC__
#define RT_HD __host__ __device__ inline
#else
#define RT_HD inline
#endif
struct alignas(64) BvhNode {
    float origin[3];
    float scale_x;
    uint32_t q[6]; // qlo_x, qhi_x, qlo_y, qhi_y, qlo_z, qhi_z
    float scale_y, scale_z;
    int32_t child[4];
    RT_HD float scale(int a) const { const float s = a == 0 ? scale_x : (a == 1 ? scale_y : scale_z); return s < 0.0f ? -s : s; }
    RT_HD void set_scale(int a, float s) { (a == 0 ? scale_x : (a == 1 ? scale_y : scale_z)) = s; }
};
static_assert(sizeof(BvhNode) == 64, "BvhNode must be 64 bytes");
constexpr int32_t kChildEmpty = (int32_t)0x80000000;
struct Box3 {
    float lo[3], hi[3];
};

// The tree's encoding rules, each written once. Words 0..11 of a node without children: the unit grid at the origin, every plane pair
// inverted (qlo = 255, qhi = 0), a miss for every ray inside the contract's range (rt_device.h: trav_inner).
RT_HD void clear_planes(BvhNode& n) {
    n.scale_x = n.scale_y = n.scale_z = 1.0f;
    n.origin[0] = n.origin[1] = n.origin[2] = 0.0f;
    for (int i = 0; i < 6; ++i) n.q[i] = (i & 1) ? 0u : 0xFFFFFFFFu;
}
RT_HD BvhNode empty_node() {
    BvhNode n;
    clear_planes(n);
    for (int k = 0; k < 4; ++k) n.child[k] = kChildEmpty;
    return n;
}
// a leaf child word <-> its records [first, first + count) of the leaf-ordered triangle array
struct LeafRange {
    uint32_t first, count;
};
RT_HD LeafRange leaf_range(int32_t child) {
    const uint32_t code = (uint32_t)~child;
    return {code >> 2, (code & 3u) + 1u};
}
RT_HD int32_t leaf_child(uint32_t first, uint32_t count) { return ~(int32_t)((first << 2) | (count - 1)); }
// the box the kernels test for child k: its quantised planes decoded (side 0: the low plane of axis a, 1: the high one)
RT_HD float child_plane(const BvhNode& n, int k, int a, int side) { return n.origin[a] + (float)((n.q[2 * a + side] >> (8 * k)) & 0xffu) * n.scale(a); }
RT_HD Box3 child_box(const BvhNode& n, int k) {
    Box3 b;
    for (int a = 0; a < 3; ++a) b.lo[a] = child_plane(n, k, a, 0), b.hi[a] = child_plane(n, k, a, 1);
    return b;
}

// In the DEVICE copy of the node array a child word >= 0 is the child node's BYTE offset (index * 64), so that the inner step
// addresses the node with no arithmetic of its own — a 32-bit offset on the scalar base for global memory (the index form cost a
// 64-bit shift and a 64-bit add per step), one right shift for the LDS copy of the tree's top. The host array keeps indices. These two
// functions are that rule (leaf codes and kChildEmpty, negative, are the same word in both forms; SkipRec::ref holds the device's form).
RT_HD uint32_t device_child_word(int32_t child) { return child >= 0 ? (uint32_t)child * 64u : (uint32_t)child; }
RT_HD int32_t host_child_word(uint32_t word) { return (int32_t)word >= 0 ? (int32_t)(word / 64u) : (int32_t)word; }
constexpr int kMaxLeafTris = 2;    // 1..4 (the leaf code keeps count - 1 in two bits). 4 -> 2: +1.1 % on the atrium — a whole-leaf step runs as many tests as the wave's LARGEST leaf
constexpr int kTopNodes = 341;    // nodes at the head of the node array laid out top first — by surface area: scene_build.cpp; by level: lbvh_gpu.hip — and staged in LDS by the traversal kernels (rt_device.h)
constexpr int kStackSize = 64;      // traversal stack entries per ray; builders keep depth < 64
constexpr uint32_t kNoTri = 0xFFFFFFFFu;
constexpr float kTNear = 0.0001f;   // RayData::to_embree tnear (src/camera.hpp:50)

// ---- range of the closest-hit contract (include/rt_mi355x.h: rt_intersect_batch) ------------------
// What the origin test needs of a scene (rt_frame.hip: contract_range): the bounds and the limit, kContractRange scene scales; finite_only
// when nothing could be culled wrongly (no geometry, or all of it in the origin). One predicate for the host entry points and the query
// kernel (rt_query.hip), written with std::max's operand order so that both evaluate the same fp32 operations with the same NaN outcome.
struct ContractRange {
    float lo[3], hi[3];
    float limit;
    uint32_t finite_only;
};
RT_HD float contract_max(float a, float b) { return a < b ? b : a; } // std::max(a, b)
RT_HD bool in_contract_range(const ContractRange& r, float ox, float oy, float oz) {
    if (r.finite_only) return __builtin_isfinite(ox) && __builtin_isfinite(oy) && __builtin_isfinite(oz);
    const float o[3] = {ox, oy, oz};
    for (int a = 0; a < 3; ++a) {
        const float outside = contract_max(contract_max(r.lo[a] - o[a], o[a] - r.hi[a]), 0.0f);
        if (!(outside <= r.limit)) return false;
    }
    return true;
}

// ---- triangles, leaf order: 48 bytes = 3 x float4 -------------------------------------------------
//   a = (v0.x, v0.y, v0.z, e1.x)  b = (e1.y, e1.z, e2.x, e2.y)  c = (e2.z, bits(global index), 0, 0)
struct alignas(16) TriRec {
    float v0[3];
    float e1[3];
    float e2[3];
    uint32_t global_index; // triangle index in rt_scene_desc order (tie-break + shading lookup)
    uint32_t pad[2];
};
static_assert(sizeof(TriRec) == 48, "TriRec must be 48 bytes");
// What the device reads per triangle: the record's ten live dwords, packed (the two padding words were 17 % of the
// triangle traffic): bytes 0-15 (v0.xyz, e1.x), 16-31 (e1.yz, e2.xy), 32-39 (e2.z, global index) at a 40-byte stride (8-byte aligned).
constexpr uint32_t kTriBytes = 40;
// record r of the packed array: its nine floats, and the word behind them
RT_HD const float* packed_tri(const uint8_t* tris, size_t r) { return reinterpret_cast<const float*>(tris + r * kTriBytes); }
RT_HD float* packed_tri(uint8_t* tris, size_t r) { return reinterpret_cast<float*>(tris + r * kTriBytes); }
RT_HD uint32_t packed_global_index(const uint8_t* tris, size_t r) { return reinterpret_cast<const uint32_t*>(tris + r * kTriBytes)[9]; }

// ---- per-triangle shading attributes, GLOBAL order: 64 bytes ------------------------------------
// What trace_ray gathers through index_buffer/normal_buffer/uv_buffer (src/trace_ray.hpp:34-45),
// pre-gathered per triangle so a hit costs one aligned 64-byte fetch instead of a dependent chain.
// `instance`: the instance index — and, in scenes with at most 2^20 instances and 2^12 materials (SceneDev::packed_mat), the instance's
// material index in bits 20..31 as well: shading then fetches the material record side by side with the instance record instead of
// after it (one hop less in the chain shade record -> instance -> material -> texel).
constexpr uint32_t kPackedInstBits = 20, kPackedInstMask = (1u << kPackedInstBits) - 1u;
struct alignas(64) ShadeRec {
    float n0[3], n1[3], n2[3];
    float uv0[2], uv1[2], uv2[2];
    uint32_t instance;
};
static_assert(sizeof(ShadeRec) == 64, "ShadeRec must be 64 bytes");

// GeometryData::obj_to_world + material id (src/scene.hpp:17-24): 48 bytes.
// Where the shading word is packed (above) the device table holds every DISTINCT normal matrix once, the one most triangles use first
// (scene_build.cpp): a glTF scene has one instance per node and primitive and a handful of different matrices — the atrium 166 and 5 —
// and shading reads the first kLdsNm of them, with the first kLdsMats materials, from LDS (rt_device.h: ShadeTables).
// (A CU's 160 KB of LDS are handed out in 1,280-byte granules — measured: k_megakernel's three workgroups per CU fit up to 53,760 bytes each,
// profiles/r05_lds_granule.txt — which leaves 1,216 bytes beside the staged tree top, the stacks and the colour sums: 8 x 48 + 24 x 32 = 1,152.)
constexpr uint32_t kLdsNm = 8, kLdsMats = 24;
struct alignas(16) InstRec {
    float normal_mat[9]; // column-major 3x3
    uint32_t material;
    uint32_t pad[2];
};
static_assert(sizeof(InstRec) == 48, "InstRec must be 48 bytes");

// Material (src/material.hpp:163-238): 48 bytes
struct alignas(16) MatRec {
    uint32_t type;
    uint32_t tex_kind;
    float color[3];
    uint32_t tex_layer;
    float emissive[3];
    float roughness;
    float ior;
    uint32_t pad;
};
static_assert(sizeof(MatRec) == 48, "MatRec must be 48 bytes");

// ---- the surface a ray starts on, GLOBAL order: 32 bytes ("the origin skip") ------------------------------------------
// A bounce ray starts on the triangle it hit, inside the padded boxes of that triangle's leaf and of every ancestor that holds nothing
// but triangles of the same plane: it would walk down to them first and test triangles that can only give t ~ 0 < kTNear. `ref` is
// the child word — as the DEVICE's parent node stores it: a node's byte offset, or a leaf code — of the highest such ancestor the
// builder has PROVEN flat (scene_check.cpp: skip_bounds), kSkipNone where there is none; the render kernels count the child with that
// word as missed for a ray whose start passes the test below.
//   n     the triangle's unit normal, computed in double and rounded to fp32 (either orientation)
//   p     the triangle's first vertex
//   a     two halves, rounded up: a0 (low) and a2 (high) of the test
//             |n . d|  >  a0 + kSkipDist * |n . (o - p)| + a2 * |o - p|_1      and      |n . d|  >  kSkipTilt * |d|_1
//         evaluated in fp32 on the origin o and the direction d the traversal uses (rt_bounce.h: origin_skip)
constexpr uint32_t kSkipNone = 1u; // no child word: a node offset is a multiple of 64, a leaf code is negative
constexpr float kSkipDist = 40400.0f;        // (4 / kTNear) x 1.01
constexpr float kSkipTilt = 1.0f / 256.0f;
struct alignas(16) SkipRec {
    uint32_t ref;
    float n[3];
    float p[3];
    uint32_t a;
};
static_assert(sizeof(SkipRec) == 32, "SkipRec must be 32 bytes");
// The test, written once for the kernels and for the host walk (scene_check.cpp: count_visits mode 4): the word a ray from o along d must not
// descend into. Every operation is a single fp32 one as written (a NaN anywhere fails both compares: kSkipNone).
RT_HD float skip_half(uint32_t bits16) {
    const uint16_t b = (uint16_t)bits16;
    _Float16 h;
    __builtin_memcpy(&h, &b, 2);
    return (float)h;
}
RT_HD uint32_t origin_skip_word(const SkipRec& e, const float o[3], const float d[3]) {
    const float wx = o[0] - e.p[0], wy = o[1] - e.p[1], wz = o[2] - e.p[2];
    const float s = __builtin_fmaf(e.n[2], wz, __builtin_fmaf(e.n[1], wy, e.n[0] * wx));
    const float nd = __builtin_fabsf(__builtin_fmaf(e.n[2], d[2], __builtin_fmaf(e.n[1], d[1], e.n[0] * d[0])));
    const float l = (__builtin_fabsf(wx) + __builtin_fabsf(wy)) + __builtin_fabsf(wz);
    const float ld = (__builtin_fabsf(d[0]) + __builtin_fabsf(d[1])) + __builtin_fabsf(d[2]);
    const float thr = __builtin_fmaf(skip_half(e.a >> 16), l, __builtin_fmaf(kSkipDist, __builtin_fabsf(s), skip_half(e.a & 0xffffu)));
    return (nd > thr && nd > kSkipTilt * ld) ? e.ref : kSkipNone;
}

// device pointers of one scene replica
struct SceneDev {
    const BvhNode* nodes;
    const uint8_t* tris; // leaf order, kTriBytes per triangle
    const ShadeRec* shade;
    const InstRec* inst;
    const MatRec* mats;
    const uint8_t* tex; // n_layers x 512 x 512 x 4
    uint32_t n_nodes;
    uint32_t n_tris;
    float sky[3];
    float cell_lo[3], cell_scale[3]; // ray re-ordering (f-3): cell = (origin - cell_lo) * cell_scale, 0..4 per axis over the scene's bounds
    uint32_t packed_mat;             // 1: ShadeRec::instance carries the material index in bits 20..31
    uint32_t lds_nm, lds_mats;       // normal matrices / materials the shading kernels stage in LDS (0: shading word not packed)
    const SkipRec* skip;             // per triangle, global order (k_megakernel and k_wf_finish only)
};

// == Camera POD (src/camera.hpp:65-72)
struct CameraDev {
    float center[3], pixel00[3], du[3], dv[3];
    int32_t width, height;
};

// image-space tile owned by this renderer (strips of `strip_rows` rows, strip k -> rank k % world)
struct TileDev {
    uint32_t rank, world, strip_rows;
    int32_t local_rows;
};

} // namespace rt
