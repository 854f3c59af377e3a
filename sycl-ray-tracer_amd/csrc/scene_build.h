// scene_build.h — host side of rt_scene: flattening instances to world-space triangles and
// building the BVH (replaces Embree's rtcCommitScene: src/scene.cpp:101-107,406-439,487-507).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_types.h"

namespace rt {

struct HostScene {
    std::vector<BvhNode> nodes;   // node 0 is the root (always an inner node)
    std::vector<TriRec> tris;     // leaf order
    std::vector<ShadeRec> shade;  // global order
    std::vector<InstRec> inst;
    std::vector<MatRec> mats;
    std::vector<uint8_t> tex;
    std::vector<float> wverts;    // 9 floats per triangle, global order (diagnostics / checks)
    std::vector<SkipRec> skip;    // global order: the subtree a ray that starts on the triangle need not enter (rt_types.h); all kSkipNone unless build_skip_table ran
    std::vector<float> rec_lo, rec_hi; // host SAH builder: per leaf record, the box of the triangle's pieces in that leaf (check_bvh)
    uint32_t n_split_triangles = 0;    // triangles the SAH builder's pre-splitting pass cut into several references
    uint32_t n_layers = 0;
    bool packed_mat = false;      // ShadeRec::instance = instance | material << 20 (rt_types.h)
    int8_t built_by = -1;         // the builder that produced `nodes`: the requested kind, or RT_BVH_MEDIAN_INTERNAL after a fallback
    float sky[3] = {0.5f, 0.7f, 1.0f};
    float bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0};
    float pad = 0.0f;             // absolute box padding used by the builder
    uint32_t max_depth = 0, max_leaf_tris = 0, stack_need = 0;
    double sah_cost = 0.0;
};

constexpr int RT_BVH_MEDIAN_INTERNAL = 99; // balanced fallback when a tree would overflow the traversal stack

// Validates `desc` and fills `out`. Returns RT_OK or RT_ERR_INVALID with `err` set.
int build_host_scene(const rt_scene_desc* desc, int bvh_kind, HostScene& out, std::string& err);

// lbvh_gpu.hip: BVH construction on the current HIP device; fills hs.nodes / hs.tris (downloaded copies).
int build_lbvh_gpu(HostScene& hs, const std::vector<TriRec>& gtris, std::string& err);

// ---- the scene-geometry rules, each written once ------------------------------------------------------------------------------------------
// World-space vertices of a triangle list under a transform table, 9 floats per triangle: world = ((m0*x + m4*y) + m8*z) + m12 per row of
// the column-major instance matrix. The expression is part of the arithmetic contract with the CPU oracle and stands here only.
void world_vertices(uint32_t n_tris, const uint32_t* indices, const uint32_t* tri_instance, const rt_instance* inst, const float* positions,
                    std::vector<float>& wv);
// Refuses non-finite vertices, reduces the rest to the scene's bounds (std::min / std::max: the first of equal values stays, the sign of a
// zero bound depends on it) and derives the box padding (scene_padding). Returns false with err set.
bool world_bounds(const std::vector<float>& wv, float lo[3], float hi[3], float& pad, std::string& err);
// rec_lo / rec_hi of every leaf record as the whole triangle's box (what a refit leaves of a pre-split triangle's pieces).
void record_boxes(HostScene& hs);
// Exact bounds of a leaf child: the union of its records' boxes — the box of the triangle's pieces in that leaf where the tree is pre-split,
// else the whole triangle's, from hs.wverts.
Box3 leaf_bounds(const HostScene& hs, int32_t child);
inline float half_area(const float* lo, const float* hi) {
    float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0.0f;
    return dx * dy + dy * dz + dz * dx;
}

// ---- dynamic scenes (rt_scene_update) ---------------------------------------------------------------------------------------------------
// The device's instance table from the instances' normal matrices (the packed shading word's distinct-matrix grouping, rt_types.h): `use`
// is the number of triangles of every instance; rows receives the table, slot[i] instance i's row.
void shading_rows(const rt_instance* inst, uint32_t n, const std::vector<uint64_t>& use, bool packed, std::vector<InstRec>& rows,
                  std::vector<uint32_t>& slot);
// The scene's bounds and box padding from the fp32 world-space vertices as min / max reduced (lo, hi): pad = 2e-5 x scene scale. Returns
// false (err set) when the padded bounds are not finite.
bool scene_padding(const float lo[3], const float hi[3], float& pad, std::string& err);
// Height levels of the node topology (height: distance to the deepest leaf below): level_nodes lists the nodes by height, level h being
// level_nodes[level_start[h] .. level_start[h + 1]). A node's children all lie in lower levels.
void node_levels(const std::vector<BvhNode>& nodes, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_start);
// Refits hs.nodes in place over hs.wverts (node topology, child words and leaf records kept): rewrites every leaf record's v0 / e1 / e2 and
// its rec_lo / rec_hi box (the whole triangle's), every node's exact child boxes (box: 6 floats per node, the union of its children) and its
// quantised words 0..11 with hs.pad, level by level, and hs.sah_cost. Returns false if a node cannot be quantised.
bool refit_host(HostScene& hs, const std::vector<uint32_t>& level_nodes, std::vector<float>& box, std::string& err);
// (scene_check.cpp) Surface-area cost of a refit tree from the nodes' exact boxes (box, 6 floats per node): inner child 1 x area, leaf child its records x
// area, relative to the root's area. A device-built tree (RT_BVH_LBVH_GPU) keeps the measure its build reported, decoded_sah_cost.
double refit_sah_cost(const HostScene& hs, const std::vector<float>& box);
// The same cost from the nodes' decoded (quantised, padded) child boxes: what a device build reports.
double decoded_sah_cost(const HostScene& hs);

// ---- the origin skip (rt_types.h: SkipRec) ------------------------------------------------------------------------------------
constexpr uint32_t kSkipMaxRecords = 128; // the largest subtree (leaf records) an entry may name: proving one flat costs a pass over it per triangle
// (scene_check.cpp) The proof behind one entry, in double: every leaf record below `child` — the triangle (v0, v0 + e1, v0 + e2) the kernels
// test — lies within `dev` of the plane through p with normal n, is no sliver (|e1||e2| / |e1 x e2| <= 256), has an area and a normal within
// 2^-10 of +-n. Returns false where that fails or the subtree holds more than kSkipMaxRecords records; else a0 and a2 of the test in rt_types.h.
bool skip_bounds(const HostScene& hs, const float n[3], const float p[3], int32_t child, double& a0, double& a2);
uint16_t half_up(double x);      // the smallest half >= x (x >= 0); 0x7C00 where there is none
float half_value(uint16_t bits);
// Fills hs.skip with kSkipNone; build_skip_table then names, per triangle, the highest ancestor skip_bounds accepts (host-built static trees only:
// rt_abi.hip leaves the table cleared for updatable scenes — vertices that move break coplanarity — and device-built trees).
void clear_skip_table(HostScene& hs);
void build_skip_table(HostScene& hs);

// ---- diagnostics (scene_check.cpp) ----------------------------------------------------------------------------------------------------------
// Structural check used by rt_scene_check_bvh.
int check_bvh(const HostScene& hs, std::string& err);

// Diagnostic used by rt_scene_count_visits: closest-hit walks on the host with quantised (0), exact (1) or finer quantised (2) child boxes; 4: as 0 with the
// origin skip of hs.skip, tri_out holding on entry the triangle every ray starts on (kNoTri: none).
int count_visits(const HostScene& hs, uint32_t n, const float* org, const float* dir, int mode, uint64_t* node_visits, uint64_t* tri_tests, float* t_out,
                 uint32_t* tri_out, std::string& err);

// Diagnostic used by rt_scene_closest_host: closest-point queries on the host (rt_closest_point.h), by brute force over the leaf records
// (use_bvh 0) or by the walk k_closest makes, counted (use_bvh 1). Any output may be NULL; max_dist2 NULL = +inf.
int closest_host(const HostScene& hs, uint32_t n, const float* pos, const float* max_dist2, int use_bvh, float* dist2, float* u, float* v, uint32_t* tri,
                 float* point, uint64_t* node_visits, uint64_t* tri_tests, std::string& err);

// Diagnostic used by rt_scene_nearest_host: k-nearest closest-point queries on the host, by brute force over the triangles in index order
// (use_bvh 0) or by the walk k_nearest makes, counted (use_bvh 1). Outputs hold k slots per point; any may be NULL; max_dist2 NULL = +inf;
// after_dist2 NULL = no key.
int nearest_host(const HostScene& hs, uint32_t n, uint32_t k, const float* pos, const float* max_dist2, const float* after_dist2,
                 const uint32_t* after_tri, int use_bvh, float* dist2, float* u, float* v, uint32_t* tri, uint32_t* count, uint64_t* node_visits,
                 uint64_t* tri_tests, std::string& err);

// Diagnostic used by rt_scene_multihit_host: multi-hit ray queries on the host, by brute force over the triangles in index order (use_bvh 0)
// or by the walk k_multihit makes, counted (use_bvh 1). Outputs hold k slots per ray; any may be NULL; tmax NULL = +inf; after_t NULL = no key.
int multihit_host(const HostScene& hs, uint32_t n, uint32_t k, const float* org, const float* dir, const float* tmax, const float* after_t,
                  const uint32_t* after_tri, int use_bvh, float* t, float* u, float* v, uint32_t* tri, uint32_t* count, uint64_t* node_visits,
                  uint64_t* tri_tests, std::string& err);

// Diagnostic used by rt_scene_occlusion_host: occlusion gathers on the host, every sample's any-hit query by brute force over the triangles
// in index order (use_bvh 0) or by the walk k_occlusion_gather makes, counted (use_bvh 1). Any output may be NULL; max_dist NULL = +inf.
int occlusion_host(const HostScene& hs, uint32_t n, uint32_t samples, const float* pos, const float* normal, const float* max_dist, const uint32_t* rng,
                   int use_bvh, uint32_t* rng_out, float* visibility, float* bent, uint32_t* clear, uint32_t* rays, uint64_t* node_visits,
                   uint64_t* tri_tests, std::string& err);

} // namespace rt
