/*
 * rt_mi355x.h — C ABI of librt_mi355x.so, the MI355X (gfx950) path-tracing hot path.
 *
 * This is the drop-in boundary for the per-pixel ray-trace loop of felipeagc/sycl-ray-tracer.
 * Every entry point names the reference interface it replaces (file:line relative to the
 * reference tree). No C++ types, no torch types, no exceptions cross this boundary: plain
 * pointers and sizes only. Every function returns RT_OK (0) or a negative rt_status;
 * rt_last_error() returns a thread-local message for the last failure.
 *
 * Threading: a renderer is used from one host thread at a time (the reference is
 * single-threaded: src/main.cpp:57-70). Different renderers may be used from different threads.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 8

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,     /* bad argument (null pointer, out-of-range index, zero size) */
    RT_ERR_NO_DEVICE = -2,   /* no usable gfx950 device / HIP runtime not functional      */
    RT_ERR_HIP = -3,         /* a HIP call failed; message carries hipGetErrorString      */
    RT_ERR_OOM = -4,         /* host or device allocation failed                          */
    RT_ERR_UNSUPPORTED = -5  /* valid request this build does not implement               */
} rt_status;

/* ---- texture array constants: src/image_manager.hpp:12-14 --------------------------------- */
#define RT_TEX_SIZE 512u      /* IMAGE_SIZE = {512,512}            */
#define RT_TEX_CHANNELS 4u    /* IMAGE_CHANNELS                     */
#define RT_TEX_MAX_LAYERS 128u /* MAX_IMAGES                        */

/* ---- Camera: the by-value POD the kernels consume, == raytracer::Camera (src/camera.hpp:65-72)
 * center / pixel00_loc / pixel_delta_u / pixel_delta_v / img_size. */
typedef struct rt_camera {
    float center[3];
    float pixel00[3];
    float delta_u[3];
    float delta_v[3];
    int32_t width;
    int32_t height;
} rt_camera;

/* Host-side camera constructor == Camera::Camera(img_size, cam_center, cam_dir, focal_length)
 * (src/camera.hpp:74-106). Pure host arithmetic; needs no GPU. */
int rt_camera_init(rt_camera* out, int32_t width, int32_t height, const float center[3],
                   const float dir[3], float focal_length);

/* ---- Materials: == raytracer::Material tagged union (src/material.hpp:56-61,163-238) ------- */
enum { RT_MAT_NONE = 0, RT_MAT_DIFFUSE = 1, RT_MAT_METALLIC = 2, RT_MAT_DIELECTRIC = 3 };
/* == TextureType (src/material.hpp:13-16) */
enum { RT_TEX_COLOR = 0, RT_TEX_IMAGE = 1 };

typedef struct rt_material {
    uint32_t type;      /* RT_MAT_*                                                        */
    uint32_t tex_kind;  /* RT_TEX_*: albedo is `color` or layer `tex_layer` of the array   */
    float color[3];     /* Texture::color  (baseColorFactor.rgb)                           */
    uint32_t tex_layer; /* ImageRef::index (src/image_manager.hpp:26-28)                   */
    float emissive[3];  /* MaterialDiffuse/Metallic::emissive; ignored for dielectric      */
    float roughness;    /* MaterialMetallic::roughness                                     */
    float ior;          /* MaterialDielectric::ior                                         */
} rt_material;          /* 44 bytes */

/* ---- Instance: one Embree instance geometry + its GeometryData (src/scene.hpp:17-24,
 * filled at src/scene.cpp:487-505). `transform` is the 4x4 column-major global matrix handed
 * to rtcSetGeometryTransform; `normal_mat` is GeometryData::obj_to_world =
 * transpose(inverse(mat3(global))) as a column-major 3x3. The index of an instance in the
 * array is Embree's instID[0] (attach order, src/scene.cpp:101-106). */
typedef struct rt_instance {
    float transform[16];
    float normal_mat[9];
    uint32_t material; /* index into rt_scene_desc::materials */
} rt_instance;         /* 104 bytes */

/* ---- Scene description: flat, caller-owned host arrays, copied during rt_scene_create.
 * Replaces what trace_ray reaches through RTCScene + GeometryData (src/trace_ray.hpp:18-45):
 *   positions/normals/uvs : object-space vertex attributes (GeometryData::vertex/normal/uv_buffer)
 *   indices               : 3 vertex indices per triangle (GeometryData::index_buffer), already
 *                           offset into the shared vertex arrays
 *   tri_instance          : instance (instID) of each triangle; triangles of one instance are
 *                           contiguous and in primID order
 *   textures              : n_layers x 512 x 512 x RGBA8, row 0 first (image_manager.hpp:76-100)
 *   sky                   : Scene::sky_color (src/scene.hpp:76) */
typedef struct rt_scene_desc {
    uint32_t n_vertices;
    const float* positions;       /* 3 * n_vertices */
    const float* normals;         /* 3 * n_vertices */
    const float* uvs;             /* 2 * n_vertices */
    uint32_t n_triangles;
    const uint32_t* indices;      /* 3 * n_triangles */
    const uint32_t* tri_instance; /* n_triangles */
    uint32_t n_instances;
    const rt_instance* instances;
    uint32_t n_materials;
    const rt_material* materials;
    uint32_t n_layers;
    const uint8_t* textures;      /* n_layers * 512*512*4, may be NULL iff n_layers == 0 */
    float sky[3];
} rt_scene_desc;

typedef struct rt_scene rt_scene;       /* opaque: device-resident flattened triangles + BVH */
typedef struct rt_renderer rt_renderer; /* opaque: ray queues, RNG states, accumulators      */

/* BVH builder selection for rt_scene_create (the image is independent of the choice). */
/*   RT_BVH_SAH      binned surface-area heuristic, built on the host (default: fastest traversal)
 *   RT_BVH_LBVH     Morton-order LBVH, built on the host
 *   RT_BVH_LBVH_GPU the same LBVH family built entirely on the device (Morton codes, radix sort, Karras tree,
 *                   refit, BVH4 collapse + quantisation): fastest build, needs device >= 0 */
enum { RT_BVH_DEFAULT = 0, RT_BVH_LBVH = 1, RT_BVH_SAH = 2, RT_BVH_LBVH_GPU = 3 };

/* Builds the world-space triangle set and the BVH, uploads everything to HIP device `device`.
 * Replaces Scene's Embree side: rtcNewScene/rtcAttachGeometry/rtcCommitScene
 * (src/scene.cpp:101-107,406-439,487-507). device < 0 builds a host-only scene (no HIP call):
 * usable with rt_scene_info / rt_scene_check_bvh only. */
int rt_scene_create(const rt_scene_desc* desc, int device, int bvh_kind, rt_scene** out);
void rt_scene_destroy(rt_scene* scene);

/* ---- Dynamic scenes (no reference counterpart here; Embree re-commits a scene whose instance matrices were changed through
 * rtcSetGeometryTransform, src/scene.cpp:491, with a refit). */
#define RT_SCENE_UPDATABLE 1u
/* == rt_scene_create, plus flags (RT_SCENE_UPDATABLE, RT_SCENE_KEEP_PREVIOUS below). RT_SCENE_UPDATABLE keeps on the device what an update needs (object positions, indices, every triangle's
 * instance, the world-space vertices, the exact box of every node and the nodes' height levels: counted in device_bytes). Unknown flag
 * bits -> RT_ERR_INVALID. */
int rt_scene_create_ex(const rt_scene_desc* desc, int device, int bvh_kind, uint32_t flags, rt_scene** out);
/* RT_SCENE_KEEP_PREVIOUS (only together with RT_SCENE_UPDATABLE, else RT_ERR_INVALID): the scene keeps a second copy of its world-space vertices
 * on the device, 9 floats per triangle (+36 bytes per triangle in device_bytes): the vertices as they were before the last accepted
 * rt_scene_update. Before the first update previous == current; an update makes the current vertices the previous ones before it writes the new
 * ones (whatever it changes: after an update of the normals alone previous == current); a refused update leaves both untouched. What reads them
 * is rt_scene_gbuffer_motion. A scene without the flag behaves exactly as before, and its updates do no extra work. */
#define RT_SCENE_KEEP_PREVIOUS 2u

typedef struct rt_scene_update_desc {
    uint32_t n_instances;         /* 0 = transforms unchanged, else == the scene's n_instances            */
    const rt_instance* instances; /* new transform + normal_mat; .material must equal the scene's        */
    uint32_t n_vertices;          /* 0 = vertices unchanged, else == the scene's n_vertices               */
    const float* positions;       /* 3 * n_vertices object-space positions, or NULL                       */
    const float* normals;         /* 3 * n_vertices object-space normals, or NULL                         */
} rt_scene_update_desc;
/* device_ms: hipEvent time of the update's device work (0 for a host-only scene); launches: kernel launches; refit_nodes: nodes refitted */
typedef struct rt_update_stats { double device_ms; uint32_t launches; uint32_t refit_nodes; } rt_update_stats;
/* Moves instances and / or vertices of a scene created with RT_SCENE_UPDATABLE, keeping its BVH's topology and refitting its boxes.
 * The contract: for an updatable scene made from desc D, rt_scene_update(S, U) makes S behave as rt_scene_create(D') would, bit for bit,
 * D' being D with U applied (the instances' transform and normal_mat, the positions, the normals). Behave means every frame under every
 * renderer, schedule, tile split and BVH kind (fp32, unorm8 and the ray count), every continuation of a frame rendered after the update,
 * rt_intersect_batch, rt_scene_info().bounds_*, the box padding (2e-5 x the scale of the new world vertices) and the contract-range check
 * on camera centres. Only the tree may differ from a fresh build: its topology is kept (child words, leaf codes, node order), so traversal
 * cost changes; rt_scene_info().sah_cost reports the refit tree's cost, so that a caller can decide when to rebuild. A triangle the SAH
 * builder pre-split sits in several leaves: after an update each of them bounds the whole triangle.
 * Refused with RT_ERR_INVALID, the scene left unchanged: a scene created without the flag, counts other than 0 or the scene's, a changed
 * material, NULL where a count is non-zero, world vertices that are non-finite or whose padded bounds overflow fp32 (rt_scene_create's
 * test), and any renderer of the scene with a frame in flight (rt_render_frame_begin without _end).
 * The call is synchronous: it returns when the device has finished. Every renderer of the scene discards its progressive state (the next
 * frame starts a new chain; continuations are refused until then, rt_renderer_accumulated_samples is 0) and re-captures its hipGraph.
 * A host-only scene (device < 0) is updated on the host with the same arithmetic. stats may be NULL. */
int rt_scene_update(rt_scene* scene, const rt_scene_update_desc* u, rt_update_stats* stats);

typedef struct rt_scene_info_t {
    uint32_t n_triangles;
    uint32_t n_nodes;
    uint32_t max_depth;     /* deepest leaf */
    uint32_t max_leaf_tris;
    float bounds_lo[3];
    float bounds_hi[3];
    double sah_cost;        /* surface-area-heuristic cost of the tree (diagnostic) */
    uint64_t device_bytes;  /* bytes resident in HBM for this scene */
    uint32_t n_leaf_records;     /* triangle records in the leaves: n_triangles, plus one per extra leaf a pre-split triangle sits in */
    uint32_t n_split_triangles;  /* triangles the SAH builder's pre-splitting pass cut into several references (large triangles whose
                                    boxes enclose much empty space; a result cannot change: closest t, ties to the lowest index) */
} rt_scene_info_t;
int rt_scene_info(const rt_scene* scene, rt_scene_info_t* out);

/* Host-side structural check of the built BVH: every triangle in exactly one leaf, every child
 * box inside its parent's, every triangle inside its leaf box. Returns RT_OK or RT_ERR_INVALID
 * (message names the first violation); every entry of the origin-skip table proven again (the triangle in the subtree it names, the
 * subtree flat on the triangle's plane within what the entry's thresholds allow). Needs no GPU. */
int rt_scene_check_bvh(const rt_scene* scene);
/* Diagnostic, host only (works on a scene built with device < 0): closest-hit walks of the tree for n rays as the traversal kernels make them
 * (children nearest first, culled by the closest hit so far), counting node visits and triangle tests, with a choice of the child boxes
 * tested: mode 0 the decoded 8-bit quantised boxes (what the kernels test), 1 the exact padded bounds of each child's subtree (what fp32
 * boxes would hold), 2 the exact bounds re-quantised with two more bits per plane, 4 (bit 2 on top of box mode 0; 3 is refused) as 0 with the origin skip of the render kernels: tri
 * (required) holds ON ENTRY the triangle each ray starts on, 0xFFFFFFFF for none, and a ray that leaves its triangle's plane steeply enough
 * does not descend into the coplanar subtree around it (profiles/origin_skip_host.txt). t / tri (may be NULL) receive the closest hits. The
 * difference between the modes is what the quantisation costs in visits on a given scene and ray set (profiles/r05_quantisation.txt). */
int rt_scene_count_visits(const rt_scene* scene, uint32_t n, const float* org, const float* dir, int mode,
                          uint64_t* node_visits, uint64_t* tri_tests, float* t, uint32_t* tri);

/* Closest-hit query for a batch of rays: the replacement for rtcIntersect1 at
 * src/trace_ray.hpp:18-27 (tnear = 1e-4, tfar = +inf, no culling, no masks).
 * org/dir: 3*n floats (host). Outputs (host, n each): t (+inf on miss), u, v and
 * tri = global triangle index in rt_scene_desc order (0xFFFFFFFF on miss).
 * Range of the contract: the result equals the brute-force closest hit over all triangles (same fp32 Moller-Trumbore) for ray
 * origins at most 100 scene scales outside the scene's bounds on any axis (scene scale = max(largest extent of the bounds, largest
 * |coordinate| of the bounds): what the padding of the BVH boxes, 2e-5 x scale, is derived from) — every ray the renderers
 * generate from a camera inside that range. Farther out the fp32 error of the ray itself (~1e-7 x |origin|) exceeds the padding and
 * a hit that only exists by that error could be culled, so the range is ENFORCED: rt_intersect_batch returns RT_ERR_INVALID (naming
 * the first offending ray) if any origin lies outside it or is not finite, and rt_render_frame* refuse such a camera centre.
 * The reference's rtcIntersect1 (src/trace_ray.hpp:18-27) states no range; this is a documented narrowing, not a silent one. */
int rt_intersect_batch(rt_scene* scene, uint32_t n, const float* org, const float* dir, float* t,
                       float* u, float* v, uint32_t* tri);

/* ---- Ray queries: closest hit and occlusion with a per-ray tmax (rtcIntersect1 / rtcOccluded1; the reference calls only the first).
 * A hit COUNTS iff 1e-4 < t <= tmax[i], with rt_intersect_batch's fp32 Moller-Trumbore test and tie-break (lowest global index at equal t).
 *   RT_QUERY_CLOSEST: the closest counting hit into t, u, v, tri — a miss (t = +inf, u = v = 0, tri = 0xFFFFFFFF) when none counts. With
 *                     tmax == NULL (+inf for every ray) that is rt_intersect_batch's result bit for bit; with a tmax it is that result when
 *                     its t <= tmax and a miss otherwise. Any of t, u, v, tri may be NULL: that output is not written.
 *   RT_QUERY_ANY:     occluded[i] = 1 iff a counting hit exists (= rt_intersect_batch hits at t <= tmax), else 0. The traversal of a ray ends
 *                     at its first counting hit.
 * Rejected rays: an origin outside the contract range or not finite (rt_intersect_batch), or a NaN tmax. rt_trace_rays returns RT_ERR_INVALID
 * naming the first of them and writes nothing; rt_trace_rays_device marks each instead — t = NaN, tri = RT_TRI_REJECTED (u, v unwritten),
 * occluded = 2 — and traces the others.
 * n == 0: RT_OK, nothing launched. RT_ERR_INVALID: NULL scene, org or dir, an unknown mode, CLOSEST with every output NULL, ANY with occluded
 * NULL; RT_ERR_NO_DEVICE: a host-only scene (the arguments are checked first).
 * rt_trace_rays takes host arrays, stages them through device buffers and synchronises. rt_trace_rays_device takes device arrays and enqueues
 * on `stream` (NULL = the null stream): no allocation, no synchronisation, no host copy. As with rt_scene_gbuffer_device, the scene records
 * an event behind the launch on each stream used and rt_scene_update waits for all of them. Query launches of one scene on different streams
 * run one after the other (they share the scene's ray cursors: the later waits for the earlier on the device, never on the host). */
enum { RT_QUERY_CLOSEST = 0, RT_QUERY_ANY = 1 };
#define RT_TRI_REJECTED 0xFFFFFFFEu
typedef struct rt_ray_query {
    uint32_t n;
    uint32_t mode;      /* RT_QUERY_*                                              */
    const float* org;   /* 3n, xyz per ray, as rt_intersect_batch                  */
    const float* dir;   /* 3n                                                      */
    const float* tmax;  /* n, or NULL = +inf for every ray                         */
    float* t;           /* CLOSEST: n each; NULL = not written                     */
    float* u;
    float* v;
    uint32_t* tri;
    uint8_t* occluded;  /* ANY: n bytes, 0 clear / 1 occluded / 2 rejected         */
} rt_ray_query;
int rt_trace_rays(rt_scene* scene, const rt_ray_query* q);
int rt_trace_rays_device(rt_scene* scene, const rt_ray_query* q, void* stream);

/* ---- Closest-point queries: the nearest triangle to caller-supplied points (probe clearance, texels under another surface, collision of
 * dynamic objects and particles, distance fields). The ABI is SQUARED throughout — no square root appears anywhere — so that a caller can
 * place a radius exactly on a result.
 * The contract (csrc/rt_closest_point.h, one text for the kernel and the host walk). For a point p and a triangle as the kernels hold it,
 * (v0, e1 = v1 - v0, e2 = v2 - v0), Ericson's region walk, every operation ONE fp32 operation evaluated left to right as bracketed, never
 * contracted; dot(a, b) = (ax*bx + ay*by) + az*bz; divisions correctly rounded:
 *     ap = p - v0;  d1 = dot(e1, ap);  d2 = dot(e2, ap)
 *     bp = ap - e1; d3 = dot(e1, bp);  d4 = dot(e2, bp)
 *     cp = ap - e2; d5 = dot(e1, cp);  d6 = dot(e2, cp)
 *     vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4
 *     the first region that holds, in this order:
 *       d1 <= 0 && d2 <= 0                         (u, v) = (0, 0)
 *       d3 >= 0 && d4 <= d3                        (1, 0)
 *       vc <= 0 && d1 >= 0 && d3 <= 0              (d1 / (d1 - d3), 0)
 *       d6 >= 0 && d5 <= d6                        (0, 1)
 *       vb <= 0 && d2 >= 0 && d6 <= 0              (0, d2 / (d2 - d6))
 *       va <= 0 && (d4-d3) >= 0 && (d5-d6) >= 0    w = (d4-d3) / ((d4-d3) + (d5-d6)); (1.0f - w, w)
 *       else                                       den = (va + vb) + vc; (vb / den, vc / den)
 *     r = (ap - u*e1) - v*e2   (per component);   dist2 = dot(r, r);   point = p - r
 * (u, v) are barycentrics along e1 / e2, as rt_intersect_batch returns them. A triangle COUNTS iff dist2 <= max_dist2[i]; a NaN dist2 never
 * counts (a degenerate triangle can give one). The winner is the lowest dist2, ties to the lowest global triangle index. The result is the
 * brute-force minimum of this expression over all triangles, bit for bit: the tree only culls.
 *   A miss (nothing counts): dist2 = +inf, u = v = 0, tri = 0xFFFFFFFF, point = three quiet NaNs.
 *   max_dist2 == NULL means +inf for every entry; a negative max_dist2 is a miss (-0.0 admits dist2 == 0).
 * THE LIMIT: the result is this arithmetic, not the real closest point. On slivers the point lies on the triangle but may not be the
 * nearest point of it (measured on the CPU: thousands of ulp of the scene scale where |e1||e2| / |e1 x e2| is about 10^4). Bounded for every
 * triangle, slivers included, is the other side: sqrt(dist2) >= d_true - 8 * 2^-24 * (|ap| + |e1| + |e2|), and the cull leans on it alone.
 * Rejected entries: a pos outside the contract range or not finite (rt_intersect_batch), or a NaN max_dist2. rt_closest_points returns
 * RT_ERR_INVALID naming the first of them and writes nothing; rt_closest_points_device marks each instead — dist2 = NaN, tri =
 * RT_TRI_REJECTED (u, v, point unwritten) — and answers the others.
 * n == 0: RT_OK, nothing launched. RT_ERR_INVALID: NULL scene, query or pos, every output NULL; RT_ERR_NO_DEVICE: a host-only scene (the
 * arguments are checked first). Any output may be NULL: it is not written.
 * rt_closest_points takes host arrays, stages them through device buffers, runs on the null stream and synchronises.
 * rt_closest_points_device takes device arrays and behaves as rt_trace_rays_device does: no allocation, no synchronisation, no host copy;
 * it shares the scene's cursors and per-stream event with the other queries, and rt_scene_update waits for it. */
typedef struct rt_point_query {
    uint32_t n;
    const float* pos;        /* 3n, xyz per point                                       */
    const float* max_dist2;  /* n squared radii, or NULL = +inf for every entry          */
    float* dist2;            /* n each; NULL = not written                              */
    float* u;
    float* v;
    uint32_t* tri;
    float* point;            /* 3n                                                      */
} rt_point_query;
int rt_closest_points(rt_scene* scene, const rt_point_query* q);
int rt_closest_points_device(rt_scene* scene, const rt_point_query* q, void* stream);
/* Diagnostic, host only (works on a scene built with device < 0; brings the host copy of an updated device scene up to date first): the
 * same queries on the host. use_bvh = 0: the brute force over the triangles with the contract's text. use_bvh = 1: the walk the kernel
 * makes — the decoded child boxes, its cull rule and child order — counting node visits and triangle tests (either may be NULL). Entries are
 * not refused here (a NaN max_dist2 is a miss); any output may be NULL; max_dist2 NULL = +inf. This is how the cull is shown conservative
 * without a GPU, and the expected side of the GPU tests. */
int rt_scene_closest_host(const rt_scene* scene, uint32_t n, const float* pos, const float* max_dist2, int use_bvh, float* dist2, float* u,
                          float* v, uint32_t* tri, float* point, uint64_t* node_visits, uint64_t* tri_tests);

/* ---- k-nearest closest-point queries: the k nearest triangles of every point, resumable (the contact set of a dynamic object or a
 * particle, "what is near this probe or this texel", smooth distance fields blended over the k nearest, every triangle within a radius:
 * the broad-phase question). rt_closest_points answers with one triangle, cannot exclude one, and no radius separates triangles that
 * tie in dist2 — coplanar neighbours share an edge's or a vertex's closest point, so ties are the common case.
 * The contract. Triangle j's candidate (dist2, u, v) for point i is rt_closest_points' text above on the record (v0, v1 - v0, v2 - v0).
 * The candidate COUNTS iff
 *     dist2 <= max_dist2[i]   and, where a resume key is given,   dist2 > after_dist2[i] || (dist2 == after_dist2[i] && j > after_tri[i])
 * — (dist2, j) > (after_dist2, after_tri) lexicographically. A NaN dist2 never counts. The answer for point i is the k smallest counting
 * candidates in ascending (dist2, j) order, in slots i * k .. i * k + k - 1 of dist2, u, v, tri (point-major). Every triangle index appears
 * at most once. count[i] is the number of slots filled; the slots past it hold rt_closest_points' miss: dist2 = +inf, u = v = 0, tri =
 * 0xFFFFFFFF. A slot is filled iff its tri is not 0xFFFFFFFF (a dist2 that overflowed to +inf counts under max_dist2 = +inf).
 * The result is the sorted brute force over all triangles, bit for bit: the tree only culls, against a bound that is max_dist2 while a
 * slot is free and the k-th entry's dist2 afterwards, by rt_closest_points' own rule. That rule leans on the candidate's underestimate
 * bound alone, which holds for slivers too: unlike rt_trace_rays_multi this query has no conditioning limit.
 *   max_dist2 == NULL means +inf for every entry; a negative max_dist2 counts nothing (-0.0 admits dist2 == 0), as for rt_closest_points.
 *   k = 1, no key:  the slot is rt_closest_points' dist2, u, v, tri bit for bit.
 *   Paging:         a page of k continued with the key (dist2, tri) of its last slot lists every counting triangle exactly once; the pages
 *                   concatenated equal one call with a larger k. The miss slot (+inf, 0xFFFFFFFF) is a key behind which nothing counts.
 *   Exhaustion:     a point with count < k has no further counting triangle.
 *   Range:          with max_dist2 = r * r the pages together are exactly the set { j : dist2_j <= r * r }.
 * There is no `point` output: r = (ap - u*e1) - v*e2 is a function of the point, the record, u and v alone, so a caller who has the
 * vertices re-forms point = p - r exactly (rtamd.bake.contact_points), and dot(r, r) is the listed dist2 bit for bit.
 * Rejected entries: a pos outside the contract range or not finite (rt_intersect_batch), a NaN max_dist2, a NaN after_dist2.
 * rt_closest_points_multi returns RT_ERR_INVALID naming the first of them and writes nothing; rt_closest_points_multi_device marks each
 * instead — all k slots dist2 = NaN and tri = RT_TRI_REJECTED (u, v unwritten), count = 0 — and answers the others.
 * Refusals, in this order: RT_ERR_INVALID for a NULL scene or query; n == 0 is RT_OK, nothing launched; then RT_ERR_INVALID for k outside
 * 1 .. RT_NEAREST_MAX, NULL pos, after_dist2 without after_tri or the reverse, every output NULL; RT_ERR_NO_DEVICE for a host-only scene
 * comes last. Any output may be NULL: it is not written.
 * rt_closest_points_multi takes host arrays, stages them through device buffers, runs on the null stream and synchronises.
 * rt_closest_points_multi_device takes device arrays and behaves as rt_closest_points_device does: no allocation, no synchronisation, no
 * host copy; it shares the scene's cursors and per-stream event with the other queries, and rt_scene_update waits for it. */
#define RT_NEAREST_MAX 8
typedef struct rt_nearest_query {
    uint32_t n, k;                        /* k in 1..RT_NEAREST_MAX, the same for every point of the call  */
    const float *pos;                     /* 3n, xyz per point                                             */
    const float *max_dist2;               /* n squared radii, or NULL = +inf                               */
    const float *after_dist2;             /* n, or NULL = no key                                           */
    const uint32_t *after_tri;            /* n; required iff after_dist2 is given                          */
    float *dist2, *u, *v; uint32_t *tri;  /* n*k each, point-major; any may be NULL, not all five outputs  */
    uint32_t *count;                      /* n                                                             */
} rt_nearest_query;
int rt_closest_points_multi(rt_scene* scene, const rt_nearest_query* q);
int rt_closest_points_multi_device(rt_scene* scene, const rt_nearest_query* q, void* stream);
/* Diagnostic, host only (works on a scene built with device < 0; brings the host copy of an updated device scene up to date first): the
 * same queries on the host. use_bvh = 0: the sorted brute force over all triangles in index order. use_bvh = 1: the walk the kernel
 * makes — the decoded child boxes culled against the moving bound, (max_dist2, 0xFFFFFFFF) while the list has free slots and (dist2, tri)
 * of its k-th entry once it is full — counting node visits and triangle tests (either may be NULL). Entries are not refused here (a NaN
 * max_dist2 or key counts nothing), k is any number >= 1 (a list longer than a point's counting triangles never fills: the walk with the
 * bound held at max_dist2), any output may be NULL. */
int rt_scene_nearest_host(const rt_scene* scene, uint32_t n, uint32_t k, const float* pos, const float* max_dist2, const float* after_dist2,
                          const uint32_t* after_tri, int use_bvh, float* dist2, float* u, float* v, uint32_t* tri, uint32_t* count,
                          uint64_t* node_visits, uint64_t* tri_tests);

/* ---- Multi-hit ray queries: the k nearest hits of every ray, resumable (wall thickness, every layer along a probe ray, X-ray picking,
 * crossing parity, interval lists). Every other ray entry point answers with at most one surface per ray; restarting a closest-hit query
 * from its hit point is not exact (the near limit swallows close layers, hits at equal t on shared edges are lost).
 * The contract. Triangle j's candidate (t, u, v) for a ray is rt_intersect_batch's fp32 Moller-Trumbore test: the fused cross and dot
 * products, the edge tests on the numerators, inv = RN(1 / det), t > 1e-4. The candidate COUNTS iff
 *     1e-4 < t <= tmax[i]   and, where a resume key is given,   t > after_t[i] || (t == after_t[i] && j > after_tri[i])
 * — (t, j) > (after_t, after_tri) lexicographically. The answer for ray i is the k smallest counting candidates in ascending (t, j)
 * order, in slots i * k .. i * k + k - 1 of t, u, v, tri (ray-major). Every triangle index appears at most once. count[i] is the number
 * of slots filled; the slots past it hold the miss values t = +inf, u = v = 0, tri = 0xFFFFFFFF. A candidate with t = +inf counts when
 * tmax is +inf (rt_intersect_batch's quirk), so a slot is filled iff its tri is not 0xFFFFFFFF, whatever isfinite(t) says.
 *   k = 1, no key:  the slot is rt_trace_rays RT_QUERY_CLOSEST bit for bit.
 *   Paging:         a page of k continued with the key (t, tri) of its last slot, for the rays whose count == k, lists every counting
 *                   hit exactly once; the pages concatenated equal one call with a larger k.
 *   Exhaustion:     a ray with count < k has no further counting hit.
 * The limit: ill-conditioned triangles. The queries reach a triangle through boxes that hold its true surface, padded by 2e-5 x the
 * scene's scale, and skip a box the ray enters behind tmax or behind the k-th entry so far. The candidate's t is the fp32 test's, and on a
 * sliver (det of the order of 1e-5 x |dir| x the edges' product) it can lie far from where the ray meets the true surface — 0.6 % of t has
 * been seen. A counting candidate whose fp32 t is more than half that padding in front of its true t may therefore be MISSING from the
 * list, when tmax or the k-th entry lies between the two. Nothing else is affected: every hit listed is a counting candidate with these
 * exact bits, in this order, at most once; a list never holds a hit the brute force would not; and on a ray all of whose counting
 * candidates lie within half the padding of their true t the list is exactly the one stated above. With such a hit on a ray, a count, a
 * crossing parity or a paged enumeration can be one short. rt_intersect_batch and rt_trace_rays have the same limit for their one hit
 * (the k = 1 identity holds regardless: both skip the same boxes). rt_scene_multihit_host with use_bvh = 0 is the list without the limit.
 * Rejected rays: an origin outside the contract range or not finite (rt_intersect_batch), a NaN tmax, a NaN after_t. rt_trace_rays_multi
 * returns RT_ERR_INVALID naming the first of them and writes nothing; rt_trace_rays_multi_device marks each instead — all k slots t = NaN
 * and tri = RT_TRI_REJECTED (u, v unwritten), count = 0 — and answers the others.
 * Refusals, in this order: RT_ERR_INVALID for a NULL scene or query; n == 0 is RT_OK, nothing launched; then RT_ERR_INVALID for k outside
 * 1 .. RT_MULTIHIT_MAX, NULL org or dir, after_t without after_tri or the reverse, every output NULL; RT_ERR_NO_DEVICE for a host-only
 * scene comes last. Any output may be NULL: it is not written.
 * rt_trace_rays_multi takes host arrays, stages them through device buffers, runs on the null stream and synchronises.
 * rt_trace_rays_multi_device takes device arrays and behaves as rt_trace_rays_device does: no allocation, no synchronisation, no host
 * copy; it shares the scene's cursors and per-stream event with the other queries, and rt_scene_update waits for it. */
#define RT_MULTIHIT_MAX 8
typedef struct rt_multihit_query {
    uint32_t n, k;                    /* k in 1..RT_MULTIHIT_MAX, the same for every ray of the call */
    const float *org, *dir;           /* 3n each, as rt_trace_rays                                  */
    const float *tmax;                /* n, or NULL = +inf                                          */
    const float *after_t;             /* n, or NULL = no key                                        */
    const uint32_t *after_tri;        /* n; required iff after_t is given                           */
    float *t, *u, *v; uint32_t *tri;  /* n*k each, ray-major; any may be NULL, not all five outputs */
    uint32_t *count;                  /* n                                                          */
} rt_multihit_query;
int rt_trace_rays_multi(rt_scene* scene, const rt_multihit_query* q);
int rt_trace_rays_multi_device(rt_scene* scene, const rt_multihit_query* q, void* stream);
/* Diagnostic, host only (works on a scene built with device < 0; brings the host copy of an updated device scene up to date first): the
 * same queries on the host. use_bvh = 0: the brute force over all triangles in index order. use_bvh = 1: the walk the kernel makes — the
 * decoded child boxes culled against the moving bound, (tmax, 0xFFFFFFFF) while the list has free slots and (t, tri) of its k-th entry once
 * it is full — counting node visits and triangle tests (either may be NULL). Rays are not refused here (a NaN tmax or key counts nothing),
 * k is any number >= 1 (a list longer than a ray's hits never fills: the walk with the bound held at tmax), any output may be NULL. */
int rt_scene_multihit_host(const rt_scene* scene, uint32_t n, uint32_t k, const float* org, const float* dir, const float* tmax,
                           const float* after_t, const uint32_t* after_tri, int use_bvh, float* t, float* u, float* v, uint32_t* tri,
                           uint32_t* count, uint64_t* node_visits, uint64_t* tri_tests);

/* ---- Path queries: radiance along caller-supplied rays (light probes, irradiance volumes, baking, reflection captures, radiance caches).
 * Entry i runs `samples` paths of at most `max_depth` rays from (org[i], dir[i]) with the renderers' own bounce (materials, textures, sky,
 * Russian roulette) on the xorshift32 state rng[i], each path continuing the state the one before left:
 *   a = rng[i]; color = (0, 0, 0)
 *   for s in 0 .. samples-1:
 *       ray: org = org[i], dir = half(dir[i]), attenuation = half(1, 1, 1), radiance = half(0, 0, 0)   (the camera ray without the camera
 *       res = (0, 0, 0)                                                                                  and without its two draws)
 *       for b in 0 .. max_depth-1:                                                   (render_pixel, src/render_megakernel.cpp:34-55)
 *           rays++; closest hit; done = the bounce's shading (draws from a)
 *           if (!done && rr_start && b+1 >= rr_start && b+1 < max_depth && !roulette(a)) break        (res stays 0)
 *           if (done) { res = result; break }
 *       color = color + res                                                          (per channel, one fp32 add; the sum starts at +0)
 *   radiance[i] = color / (float)samples;  rng_out[i] = a;  rays[i] = rays
 * Nothing is clamped and no square root is taken: the caller owns the estimator. A frame of the renderers is exactly a chain of path queries:
 * per pixel, seed the state as the renderer does, and per sample draw the camera ray's two jitter values from it, trace samples = 1 with the
 * state, add the radiance (the wavefront renderer clamps every sample to [0, 1] first); sqrt(sum / spp) is the frame bit for bit.
 * Rejected rays: an origin outside the contract range or not finite, as for rt_trace_rays. rt_trace_paths returns RT_ERR_INVALID naming the
 * first of them and writes nothing; rt_trace_paths_device marks each — radiance = three NaNs, rays = 0xFFFFFFFF, rng_out[i] = rng[i] — and
 * traces the others.
 * n == 0: RT_OK, nothing launched. RT_ERR_INVALID: NULL scene or query, NULL org, dir, rng or radiance, max_depth == 0, samples == 0;
 * RT_ERR_NO_DEVICE: a host-only scene (the arguments are checked first). Aliasing: rng_out == rng is allowed, nothing else.
 * rt_trace_paths takes host arrays, stages them through device buffers and synchronises. rt_trace_paths_device takes device arrays and enqueues
 * on `stream` (NULL = the null stream): no allocation, no synchronisation, no host copy. It records the scene's per-stream event, so
 * rt_scene_update waits for it, and it shares the scene's ray cursors with the ray queries: path- and ray-query launches of one scene on
 * different streams run one after the other (the later waits for the earlier on the device).
 * Limits: no per-ray tmin or tmax on the first segment; no per-ray depth; no camera model (the caller generates the rays); directions pass
 * through half precision, as every ray of the renderers does; a direction that half stores as (0, 0, 0) (every |component| <= 2^-25) or with an
 * infinite component (|component| >= 65520) hits nothing: each of the entry's paths is the sky after one ray, and no draw is taken; the
 * paths of one entry repeat the same first segment (a caller who wants jitter issues samples = 1 calls); multi-GPU is the caller's split of the ray list across scene replicas. */
typedef struct rt_path_query {
    uint32_t n;
    uint32_t max_depth;     /* >= 1: rays per path at most, as rt_renderer_create's            */
    uint32_t samples;       /* >= 1: paths per ray                                             */
    uint32_t rr_start;      /* rt_renderer_set_russian_roulette's start_bounce; 0 = off        */
    const float* org;       /* 3n, fp32                                                        */
    const float* dir;       /* 3n, fp32; stored as three halves, as the renderers' rays are    */
    const uint32_t* rng;    /* n: every ray's xorshift32 state before its first path           */
    uint32_t* rng_out;      /* n: the state after its last path; may be NULL, may be == rng    */
    float* radiance;        /* 3n: linear radiance                                             */
    uint32_t* rays;         /* n or NULL: rays traced for this entry (the frame's ray count)   */
} rt_path_query;
int rt_trace_paths(rt_scene* scene, const rt_path_query* q);
int rt_trace_paths_device(rt_scene* scene, const rt_path_query* q, void* stream);

/* ---- Gather queries: diffuse-lobe radiance at caller-supplied points (lightmap texels, mesh vertices, the faces of ambient-cube probes).
 * Entry i runs `samples` paths from pos[i], each with a direction of its own: the diffuse bounce's scattered direction about normal[i]
 * (MaterialDiffuse::scatter, src/material.hpp:72-86, without its near_zero clause: there is no incoming direction), drawn from the entry's
 * xorshift32 state. From that ray on a path is rt_trace_paths' path, same loop, same roulette rule, on the same running state:
 *   a = rng[i]; color = (0, 0, 0)
 *   for s in 0 .. samples-1:
 *       u = random_unit_vector(a)        (three draws x, y, z, each -1 + 2 * next(a); v * (1 / sqrt(dot(v, v))), R1 / R2 of DESIGN.md §3)
 *       d = normal[i] + u                (one fp32 add per component)
 *       ray: org = pos[i], dir = half(d), attenuation = half(1, 1, 1), radiance = half(0, 0, 0)
 *       res = the path of rt_trace_paths from that ray (rays++ per closest-hit query, draws from a)
 *       color = color + res              (per channel, one fp32 add; the sum starts at +0)
 *   radiance[i] = color / (float)samples;  rng_out[i] = a;  rays[i] = rays
 * The state goes in and comes out, so a gather is bit for bit a chain of path queries: per sample draw u from the state, call rt_trace_paths
 * with (pos[i], normal[i] + u), samples = 1 and the state, add the radiance. The result is what a white Lambertian surface at pos[i] with
 * shading normal normal[i] would scatter, in the renderers' own arithmetic: albedo x result is what the renderers show for that surface's
 * first diffuse bounce. Six entries with the axis normals at one point are an ambient cube.
 * Rejected entries: a pos outside the contract range or not finite (as rt_trace_paths' origin), or a normal component that is not finite.
 * rt_gather_paths returns RT_ERR_INVALID naming the first of them and writes nothing; rt_gather_paths_device marks each — radiance = three NaNs,
 * rays = 0xFFFFFFFF, rng_out[i] = rng[i], no draw taken — and traces the others.
 * n == 0: RT_OK, nothing launched. RT_ERR_INVALID: NULL scene or query, NULL pos, normal, rng or radiance, max_depth == 0, samples == 0;
 * RT_ERR_NO_DEVICE: a host-only scene (the arguments are checked first). Aliasing: rng_out == rng is allowed, nothing else.
 * rt_gather_paths takes host arrays, stages them through device buffers and synchronises. rt_gather_paths_device takes device arrays and
 * enqueues on `stream` (NULL = the null stream): no allocation, no synchronisation, no host copy. It records the scene's per-stream event, so
 * rt_scene_update waits for it, and it shares the scene's ray cursors with the ray and path queries: query launches of one scene on different
 * streams run one after the other (the later waits for the earlier on the device).
 * A direction that half stores as (0, 0, 0) or with an infinite component (a finite normal of 1e5, say) hits nothing: that path is the sky
 * after one ray, and its three direction draws are still taken.
 * Limits: the lobe is the renderers' lobe. random_unit_vector is a normalised sample of the cube [-1, 1]^3, not a uniform sample of the sphere,
 * so pi x result is the irradiance only as far as the reference's own diffuse bounce is cosine-weighted: a kept quirk, not a bug. The normal
 * is used as given, not normalised: its length shapes the lobe. An entry is sequential work on one lane: fewer than about (resident lanes)
 * entries under-fill the device, so a caller with few points and many samples passes each point several times with different states and
 * averages. There is no per-entry samples, tmin or tmax. */
typedef struct rt_gather_query {
    uint32_t n;
    uint32_t max_depth;     /* >= 1, as rt_path_query's                                  */
    uint32_t samples;       /* >= 1: paths per entry, each with a direction of its own   */
    uint32_t rr_start;      /* as rt_path_query's; 0 = off                               */
    const float* pos;       /* 3n: where the paths start                                 */
    const float* normal;    /* 3n: the lobe's axis, used as given (not normalised)       */
    const uint32_t* rng;    /* n                                                         */
    uint32_t* rng_out;      /* n or NULL; may be == rng                                  */
    float* radiance;        /* 3n: mean radiance over the entry's paths                  */
    uint32_t* rays;         /* n or NULL                                                 */
} rt_gather_query;
int rt_gather_paths(rt_scene* scene, const rt_gather_query* q);                       /* host arrays  */
int rt_gather_paths_device(rt_scene* scene, const rt_gather_query* q, void* stream);  /* device arrays */

/* ---- Occlusion gathers: ambient occlusion and the bent normal at caller-supplied points (AO lightmaps and vertex AO, sky-visibility masks
 * for probe placement, contact darkening, the visibility term beside SH probes). Visibility is the share of the renderers' diffuse lobe
 * about normal[i] that is free of geometry within max_dist[i]; the bent normal is the mean unoccluded direction. Where a gather is a chain
 * of path queries, an occlusion gather is a chain of RT_QUERY_ANY ray queries. Every operation is one fp32 operation of DESIGN.md §3,
 * evaluated left to right as bracketed, never contracted:
 *   a = rng[i]; clear = 0; rays = 0; sum = (+0, +0, +0)
 *   for s in 0 .. samples-1:
 *       u  = random_unit_vector(a)                   (rt_gather_paths' three draws, always taken)
 *       d  = normal[i] + u                           (one add per component: the renderers' diffuse lobe, as rt_gather_paths')
 *       l2 = (d.x*d.x + d.y*d.y) + d.z*d.z
 *       if !(l2 > 0) or l2 is not finite:            a DEGENERATE sample: no ray; clear++; nothing added to sum
 *       else:
 *           w = d * (1 / sqrt(l2))                   (random_unit_vector's own normalisation, R1 / R2)
 *           rays++
 *           occluded = rt_trace_rays RT_QUERY_ANY on org = pos[i], dir = w (fp32, NOT through half), tmax = max_dist[i]
 *           if !occluded: clear++; sum = sum + w     (per component, in sample order)
 *   visibility[i] = (float)clear / (float)samples
 *   bent[i]       = sum / (float)samples             (per component; not normalised: its length is the caller's confidence)
 *   clear[i] = clear;  rays[i] = rays;  rng_out[i] = a
 * max_dist == NULL means +inf for every entry. Directions are unit vectors, so max_dist is a distance in world units. A negative
 * max_dist occludes nothing; its rays are still counted (-0.0 and 0 occlude nothing either: a hit has t > 1e-4).
 * The state goes in and comes out, so an occlusion gather is bit for bit a chain of rt_trace_rays RT_QUERY_ANY calls, and inherits the
 * one limit every ray query here shares, the ill-conditioned triangle whose fp32 t straddles tmax: stated at rt_multihit_query above and
 * in DESIGN.md §14 and §24. rt_scene_occlusion_host with use_bvh = 0 is the gather without that limit.
 * The lobe is the renderers' lobe, quirk included: random_unit_vector is a normalised sample of the cube [-1, 1]^3 (rt_gather_query's
 * limits), so visibility is ambient occlusion in the same measure in which albedo x rt_gather_paths is the first diffuse bounce. The
 * normal is used as given, not normalised.
 * Rejected entries: a pos outside the contract range or not finite (rt_trace_rays' origin), a normal component that is not finite, a NaN
 * max_dist. rt_gather_occlusion returns RT_ERR_INVALID naming the first of them and writes nothing; rt_gather_occlusion_device marks each
 * instead — visibility = NaN, bent = three NaNs, clear = rays = 0xFFFFFFFF, rng_out[i] = rng[i], no draw taken — and answers the others.
 * Refusals, in this order: RT_ERR_INVALID for a NULL scene or query; n == 0 is RT_OK, nothing launched; then RT_ERR_INVALID for samples
 * == 0 or samples > RT_OCCLUSION_MAX_SAMPLES (the limit keeps (float)clear exact and bounds the time one lane spends on one entry), for a
 * NULL pos, normal or rng, for visibility, bent, clear and rays all NULL; RT_ERR_NO_DEVICE for a host-only scene comes last. Any single
 * output may be NULL: it is not written. Aliasing: rng_out == rng is allowed, nothing else.
 * rt_gather_occlusion takes host arrays, stages them through device buffers, runs on the null stream and synchronises.
 * rt_gather_occlusion_device takes device arrays and behaves as rt_trace_rays_device does: no allocation, no synchronisation, no host
 * copy; it shares the scene's cursors and per-stream event with the other queries, and rt_scene_update waits for it.
 * Limits: one `samples` for the call; no uniform-hemisphere or cone lobe; no mean hit distance (an any-hit query ends at its first hit);
 * no normal-offset bias (the caller moves pos); an entry is sequential work on one lane, as rt_gather_paths'. */
#define RT_OCCLUSION_MAX_SAMPLES 65535
typedef struct rt_occlusion_query {
    uint32_t n, samples;     /* samples in 1..RT_OCCLUSION_MAX_SAMPLES, the same for every entry     */
    const float* pos;        /* 3n: where the rays start                                             */
    const float* normal;     /* 3n: the lobe's axis, used as given (not normalised)                  */
    const float* max_dist;   /* n, or NULL = +inf for every entry                                    */
    const uint32_t* rng;     /* n: every entry's xorshift32 state                                    */
    uint32_t* rng_out;       /* n or NULL; may be == rng                                             */
    float* visibility;       /* n: clear / samples                                                   */
    float* bent;             /* 3n: the sum of the unoccluded directions / samples                   */
    uint32_t* clear;         /* n: samples that met nothing (degenerate ones included)               */
    uint32_t* rays;          /* n: rays traced (samples - degenerate ones)                           */
} rt_occlusion_query;        /* 80 bytes */
int rt_gather_occlusion(rt_scene* scene, const rt_occlusion_query* q);                       /* host arrays  */
int rt_gather_occlusion_device(rt_scene* scene, const rt_occlusion_query* q, void* stream);  /* device arrays */
/* Diagnostic, host only (works on a scene built with device < 0; brings the host copy of an updated device scene up to date first): the
 * same gather on the host, q's arrays being host arrays. use_bvh = 0: every sample's query by brute force over all triangles in index
 * order with rt_scene_multihit_host's fp32 candidate. use_bvh = 1: the any-hit walk the kernel makes — the decoded child boxes culled
 * against max_dist, nearest child first, over at the first leaf that holds a counting hit — counting node visits and triangle tests
 * (either may be NULL). Entries are not refused here (a NaN max_dist occludes nothing, a normal that is not finite makes every sample
 * degenerate); samples is checked as above; any output may be NULL. */
int rt_scene_occlusion_host(const rt_scene* scene, const rt_occlusion_query* q, int use_bvh, uint64_t* node_visits, uint64_t* tri_tests);

/* ---- Lightmap baking: the atlas-side half of a bake around one gather query, on one stream. A lightmap is a W x H atlas over one scene with
 * one lightmap UV per triangle corner: lm_uv holds 6 floats per triangle in the scene's global triangle order, corner 0, 1, 2 as (u, v),
 * copied at creation. Texel i = y * W + x; (u, v) = (0, 0) is the corner of texel (0, 0); nothing wraps. Every operation below is one R1 fp32
 * operation of DESIGN.md §3, left to right as bracketed, never contracted.
 *   1. Coverage. Corner k in texel space: P_k = (u_k * (float)W, v_k * (float)H); the texel's centre c = ((float)x + 0.5f, (float)y + 0.5f).
 *      E(A, B, q) = (B.x - A.x) * (q.y - A.y) - (B.y - A.y) * (q.x - A.x). The value of the directed edge P_i -> P_j at q is E(P_i, P_j, q) if
 *      P_i comes first in the order (x, then y; P_i.x < P_j.x, or equal and P_i.y <= P_j.y), else -E(P_j, P_i, q): two triangles that share
 *      an edge with bit-identical corners see exact negatives, so no centre between them is lost and none needs a tolerance.
 *      area = edge(P_0 -> P_1) at P_2; e0, e1, e2 = the edges P_1 -> P_2, P_2 -> P_0, P_0 -> P_1 at c. Triangle t covers the texel iff its six
 *      texel-space coordinates are finite, area != 0, and e0, e1, e2 are all >= 0 (area > 0) or all <= 0 (area < 0); a NaN value covers
 *      nothing (UVs of 1e30 overflow to that). The texel's owner is the LOWEST covering triangle index; 0xFFFFFFFF: none.
 *   2. Guides, for the owner: bx = e1 / area, by = e2 / area, w = (1.0f - bx) - by, no clamp. pos = (b[k] * w + b[3 + k] * bx) + b[6 + k] * by
 *      over the triangle's nine world-space vertex floats b (rt_scene_gbuffer_motion's expression). normal = rt_scene_gbuffer's: the vertex
 *      normals as normalize((w * n0 + bx * n1) + by * n2), through the instance's normal matrix, normalised again. An empty texel has pos =
 *      three quiet NaNs (0x7FC00000) and normal = 0.
 *   3. Entries. Texel i and repeat k make entry e = i * repeats + k with texel i's pos and normal and the state
 *      (seed + (e + 1) * 0x9E3779B9) mod 2^32, 0 replaced by 0x9E3779B9.
 *   4. One rt_gather_paths_device over the W * H * repeats entries (samples, max_depth, rr_start as given). Empty texels are rejected there by
 *      their position: a claim, no ray.
 *   5. Resolve. A texel is SAMPLED iff it has an owner and none of its entries was rejected (vertex normals of zero make a NaN normal, which is).
 *      Sampled: total = +0, total = total + radiance[i * repeats + k] for k in order, rgb = total / (float)repeats, alpha 1. Else (0, 0, 0, 0).
 *   6. `dilate` passes, ping-pong: a texel with alpha 0 in the pass's input looks at dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), the centre
 *      and taps outside the atlas skipped; over the taps with alpha > 0, S += rgb in tap order from +0, n counted; n > 0: rgb = S / (float)n,
 *      alpha 0.5. Every other texel is copied. So alpha 1 = sampled, 0.5 = filled by dilation, 0 = still empty.
 *   7. Stats: covered = texels with an owner, sampled as in 5, filled = texels with alpha 0.5 at the end, rays = the sum of the gather's ray
 *      counts over the entries not rejected. d_stats holds the same 24 bytes.
 * Nothing here multiplies by an albedo or adds emission: albedo x lightmap is the caller's, as for the gather.
 * rt_lightmap_texels[_device] return steps 1 and 2: tri (W*H uint32), pos and normal (3*W*H floats each); any may be NULL, not all three.
 * rt_lightmap_bake[_device] run steps 1 to 7 into out_rgba (W*H*4 floats; the device pointer 16-byte aligned); stats / d_stats may be NULL.
 * The lightmap owns every device buffer it needs, allocated by rt_lightmap_create: no later call allocates on the device. Per triangle: the
 * UV copy, 24 bytes, and for a scene without RT_SCENE_UPDATABLE a copy of its world-space vertices, 36 bytes (an updatable scene's own are
 * read in place, so a bake after rt_scene_update sees the moved geometry). Per texel: the owner plane (4) and two float4 planes (32), and per
 * entry, max_repeats of them per texel, pos, normal, state, radiance and ray count (12 + 12 + 4 + 12 + 4): 36 + 44 * max_repeats bytes.
 * The host forms synchronise; the device forms enqueue on `stream` (NULL = the null stream) and return. Calls on one lightmap are serialised
 * by the lightmap: each records an event that the next call's stream waits for. Every call records the scene's per-stream event behind its
 * last kernel that reads the scene's geometry, so rt_scene_update waits for it. A lightmap is destroyed before its scene, as a renderer is.
 * Refused with RT_ERR_INVALID, before any HIP call: NULL handles or required pointers, W or H outside 1 .. 8192, max_repeats == 0,
 * W * H * max_repeats >= 2^31, samples == 0, max_depth == 0, repeats == 0, repeats > max_repeats, dilate > 16. After these,
 * rt_lightmap_create returns RT_ERR_NO_DEVICE for a host-only scene.
 * Limits: a texel is its centre (no conservative rasterisation, no supersampling inside a texel); there is no chart packer and no reading of
 * a second UV set from a file; one device. A filtered lightmap (below) is biased: it trades variance for blur across shadow edges narrower
 * than a texel's noise.
 *
 * Lightmap filtering, for a lightmap created by rt_lightmap_create_ex with RT_LIGHTMAP_FILTER (rt_lightmap_create is rt_lightmap_create_ex
 * with flags 0: the same allocation, the same behaviour; an unknown flag is RT_ERR_INVALID). The `repeats` entries of a texel are independent
 * estimates, so their spread is an unbiased variance of the texel's mean, and the texel's world position and shading normal (step 2) are the
 * edge-stopping guides of an a-trous filter in texel space: texels that are neighbours in the world filter together whichever chart they lie
 * on, texels that are neighbours only in the atlas do not. lum, dot, exp_m, coefficient, h[5], k3[3] and the 1e-8f are rt_denoise_guided's;
 * every operation is one R1 fp32 operation, left to right as bracketed, never contracted.
 * rt_lightmap_bake_filtered[_device] are rt_lightmap_bake's steps 1 to 7 with two steps between 5 and 6:
 *   5a. Variance. A sampled texel with entries r_k (k = 0 .. R-1, R = repeats): l_k = lum(r_k); m = (the sum of l_k in order from +0) / (float)R;
 *       s = the sum of (l_k - m) * (l_k - m) in order from +0; var = s / ((float)R * (float)(R - 1)): the variance of the texel's mean luminance.
 *       R = 1: var = 0. Not sampled: var = 0.
 *   5b. Filter. The mask M is "sampled". For i = 0 .. iterations-1 with step s = 2^i, at every texel p = (x, y) in M:
 *       a. g_p = G / K. G sums (k3[dy+1] * k3[dx+1]) * var_q and K the same kernel weights, both from +0 over dy = -1 .. 1 (outer), dx = -1 .. 1
 *          (inner), over the taps q = (x + dx, y + dy) that lie inside the atlas and in M: nothing is clamped, nothing is scaled by the step,
 *          and the centre is always in, so K >= 1/4. kl_p = 1 / (sigma_luminance * sqrt(g_p) + 1e-8f).
 *       b. The taps are q = (x + s*dx, y + s*dy), dy = -2 .. 2 (outer), dx = -2 .. 2 (inner); a tap outside the atlas or not in M is skipped.
 *          E = (fabs(l_p - l_q) * kl_p + dot(N_p - N_q) * kn_i) + dot(P_p - P_q) * kx, l = lum(L), kn_i = ldexp(kn, -2i), kn and kx the
 *          coefficients of sigma_normal and sigma_position; a term whose coefficient is 0 is left out, and E starts at +0. With
 *          sigma_luminance = +inf step a and the luminance term are left out. w = (h[dy+2] * h[dx+2]) * exp_m(-E).
 *       c. In tap order: S += w * L_q, Wsum += w, V += (w * w) * var_q; then L' = S / Wsum, var' = V / (Wsum * Wsum). L and var are linear
 *          radiance throughout: no square and no square root anywhere.
 *       A texel outside M stays (0, 0, 0) with var 0 and contributes to nothing. After the last iteration alpha is 1 on M and 0 elsewhere, and
 *       the dilation (step 6) runs on the filtered plane. out_variance (W*H floats; may be NULL) is var' on M and 0 elsewhere, filled texels
 *       included.
 *   With iterations == 0, or with the filter parameters NULL, out_rgba and the stats are rt_lightmap_bake's bit for bit and out_variance is 5a's.
 * rt_lightmap_filter[_device] are step 5b alone on the caller's planes: rgba W*H*4 floats, variance W*H floats (NULL only with sigma_luminance
 * = +inf: the variance is then 0 throughout). M is "rgba's alpha == 1.0f, the texel has an owner, and its six guide floats are finite". The
 * guides are the lightmap's own: the call runs steps 1 and 2 first, so a call after rt_scene_update sees the moved geometry, and it records
 * the scene's per-stream event as rt_lightmap_texels_device does. A texel outside M comes out (0, 0, 0, 0) with variance 0; there is no
 * dilation; iterations == 0 copies (alpha 1 on M, zeros elsewhere). out_rgba may alias rgba; nothing else may alias. out_variance may be NULL.
 * The 3 x 3 variance prefilter of step a has no guides: where two charts touch in the atlas it mixes the variances of both sides into g_p,
 * which scales the luminance term there and moves no radiance across (a gutter of one texel between charts keeps it apart).
 * Non-finite radiance or variance does what the arithmetic gives, as in rt_denoise_guided: the filter does not clamp (a NaN or negative
 * variance under a texel's 3 x 3 window makes kl_p NaN, every weight of that texel 0 and the texel NaN; an infinite radiance spreads as NaN).
 * RT_LIGHTMAP_FILTER adds 56 bytes per texel to the lightmap's buffers, allocated at creation like the others: two float4 guide planes,
 * position with the mask in .w and normal (32: a tap is two aligned 16-byte loads beside its colour, whose .w carries the variance between
 * iterations), and the host forms' staging, an rgba plane (16) and a variance plane in and out (4 + 4).
 * Refused with RT_ERR_INVALID, before any HIP call and before the handle is looked at: iterations > 10; a sigma that is NaN or below 1e-6;
 * rt_lightmap_bake_filtered with iterations > 0, a finite sigma_luminance and repeats < 2 (one entry has no noise estimate);
 * rt_lightmap_filter with variance NULL and a finite sigma_luminance. Then: a lightmap created without RT_LIGHTMAP_FILTER.
 * The four calls are serialised by the lightmap's event as the others are; the host forms run on the lightmap's stream and synchronise, the
 * device forms (device pointers, 16-byte aligned planes) enqueue on `stream` and return. */
typedef struct rt_lightmap rt_lightmap;
typedef struct rt_lightmap_params { uint32_t samples, max_depth, rr_start, repeats, seed, dilate; } rt_lightmap_params; /* 24 bytes */
typedef struct rt_lightmap_stats  { uint32_t covered, sampled, filled, reserved; uint64_t rays; } rt_lightmap_stats;    /* 24 bytes */
int  rt_lightmap_create(rt_scene* scene, int32_t width, int32_t height, uint32_t max_repeats, const float* lm_uv, rt_lightmap** out);
void rt_lightmap_destroy(rt_lightmap* lm);
int  rt_lightmap_texels(rt_lightmap* lm, uint32_t* tri, float* pos, float* normal);                       /* host arrays, synchronises */
int  rt_lightmap_texels_device(rt_lightmap* lm, void* d_tri, void* d_pos, void* d_normal, void* stream);  /* device arrays, enqueues    */
int  rt_lightmap_bake(rt_lightmap* lm, const rt_lightmap_params* p, float* out_rgba, rt_lightmap_stats* stats);
int  rt_lightmap_bake_device(rt_lightmap* lm, const rt_lightmap_params* p, void* d_out_rgba, void* d_stats, void* stream);
#define RT_LIGHTMAP_FILTER 1u
typedef struct rt_lightmap_filter_params {
    uint32_t iterations;    /* 0 .. 10; 0 = no filter                                              */
    float sigma_luminance;  /* in standard deviations; >= 1e-6, +inf = term off                    */
    float sigma_normal;     /* >= 1e-6, +inf = off                                                 */
    float sigma_position;   /* world units; >= 1e-6, +inf = off                                    */
} rt_lightmap_filter_params; /* 16 bytes */
int  rt_lightmap_create_ex(rt_scene* scene, int32_t width, int32_t height, uint32_t max_repeats, const float* lm_uv, uint32_t flags,
                           rt_lightmap** out);
int  rt_lightmap_bake_filtered(rt_lightmap* lm, const rt_lightmap_params* p, const rt_lightmap_filter_params* f, float* out_rgba,
                               float* out_variance, rt_lightmap_stats* stats);
int  rt_lightmap_bake_filtered_device(rt_lightmap* lm, const rt_lightmap_params* p, const rt_lightmap_filter_params* f, void* d_out_rgba,
                                      void* d_out_variance, void* d_stats, void* stream);
int  rt_lightmap_filter(rt_lightmap* lm, const rt_lightmap_filter_params* f, const float* rgba, const float* variance, float* out_rgba,
                        float* out_variance);
int  rt_lightmap_filter_device(rt_lightmap* lm, const rt_lightmap_filter_params* f, const void* d_rgba, const void* d_variance,
                               void* d_out_rgba, void* d_out_variance, void* stream);

/* ---- Irradiance probe volumes: nine spherical-harmonic coefficients (bands 0 to 2) of the arriving radiance at every probe of a regular
 * grid, baked around one path query on one stream, and sampled at caller-supplied points: light for what has no parametrisation of its own
 * (moving objects, particles, a mesh dropped into a baked scene). Probe p = (iz * count[1] + iy) * count[0] + ix sits at
 * origin + ((float)ix, (float)iy, (float)iz) * spacing, one fp32 multiply and one add per axis. A table is probes * 9 float4: coefficient k
 * of probe p at float4 p * 9 + k, rgb in .xyz; the .w of coefficient 0 is the probe's validity (1.0f or 0.0f), the other .w are 0, so one
 * probe is 144 contiguous bytes. Every operation below is one R1 fp32 operation of DESIGN.md §3, left to right as bracketed, never
 * contracted; sqrt and the divisions are correctly rounded; there is no transcendental function. next(a) is the renderers' xorshift32 draw.
 *   1. Entries. Probe p and direction j make entry e = p * dirs + j with the probe's position and the state
 *      (seed + (e + 1) * 0x9E3779B9) mod 2^32, 0 replaced by 0x9E3779B9 (the lightmap's rule).
 *   2. Direction, uniform on the sphere (Marsaglia 1972), drawn from the entry's state a. At most 8 tries: x1 = -1.0f + 2.0f * next(a), then
 *      x2 likewise, s = x1 * x1 + x2 * x2; the first try with s < 1.0f ends them. If all 8 were rejected (about 4.5e-6 of the entries), the
 *      last pair is scaled, x1 = x1 * 0.70710677f and x2 likewise, and s recomputed: it is then at most 1, and the 16 draws stay taken.
 *      r = sqrt(1.0f - s); d = ((2.0f * x1) * r, (2.0f * x2) * r, 1.0f - 2.0f * s). The state after these draws is the entry's path state.
 *   3. Paths. One rt_trace_paths_device over the probes * dirs entries (org = the position, dir = d, rng = the path state): samples = 1,
 *      max_depth and rr_start as given, rng_out NULL, rays kept. A probe outside the contract range is rejected there, all its entries
 *      together; it is then INVALID: its nine coefficients are 0 and its validity is 0.
 *   4. Projection. For a valid probe, coefficient k and channel c: C = +0; for j = 0 .. dirs-1 in order, C = C + radiance[e][c] * Y_k(d_e),
 *      d_e the fp32 direction of step 2 (not the half the path query stores); coef = C * (12.566371f / (float)dirs). With (x, y, z) = d:
 *        Y0 = 0.2820948f                Y1 = 0.48860252f * y             Y2 = 0.48860252f * z
 *        Y3 = 0.48860252f * x           Y4 = 1.0925485f * (x * y)        Y5 = 1.0925485f * (y * z)
 *        Y6 = 0.31539157f * (3.0f * (z * z) - 1.0f)                      Y7 = 1.0925485f * (x * z)
 *        Y8 = 0.54627424f * (x * x - y * y)
 *      One lane owns one (probe, k) and sums its directions in order: no cross-lane reduction, no atomics. Non-finite radiance does what
 *      the arithmetic gives.
 *   5. Stats: probes, valid, and rays = the sum of the entries' ray counts over the valid probes. d_stats holds the same 16 bytes.
 *   6. Sample, per point q with normal n (used as given, as the gather's is). Per axis: g = (q - origin) / spacing, g = fmin(fmax(g, 0.0f),
 *      (float)(count - 1)); i0 = min((int)g, count - 2), or 0 when count == 1; f = g - (float)i0; the weights are (1.0f - f, f). The eight
 *      corners in z-outer, y, x-inner order, corner weight w = (wx * wy) * wz; an invalid probe, and the upper corner of an axis with
 *      count == 1, are skipped. W and S_k (per channel) sum w and w * coef_k in corner order from +0; C_k = S_k / W; W == 0 gives (0, 0, 0).
 *      E = +0; for k = 0 .. 8: E = E + (B_k * C_k) * Y_k(n), B = 1.0f (k = 0), 0.6666667f (k = 1 .. 3), 0.25f (k = 4 .. 8): Ramamoorthi and
 *      Hanrahan's cosine-lobe factors over pi. out = fmaxf(E, 0.0f). A point or normal with a component that is not finite gives three NaNs.
 * The result is irradiance over pi: what a white Lambertian surface there would scatter. albedo x result is the caller's, the convention of
 * the gather and the lightmap. A point outside the volume is clamped onto it.
 * rt_probe_volume_entries[_device] return steps 1 and 2: pos, dir (3 * probes * dirs floats each) and state (probes * dirs words); any may be
 * NULL, not all three. rt_probe_volume_bake[_device] run steps 1 to 5; the table stays in the volume, and out_sh (probes * 36 floats; the device
 * pointer 16-byte aligned) receives a copy when it is not NULL; stats / d_stats may be NULL. rt_probe_volume_set_sh[_device] load a table
 * (a saved bake, or a synthetic one) and rt_probe_volume_get_sh[_device] copy it out. rt_probe_volume_sample[_device] run step 6 on n points:
 * pos, normal and out_rgb are 3n floats each; n == 0 is RT_OK with nothing launched.
 * The volume owns every device buffer it needs, allocated by rt_probe_volume_create: no later call allocates. Per entry, max_dirs of them per
 * probe: pos, dir, state, radiance and ray count (12 + 12 + 4 + 12 + 4 = 44 bytes); per probe the table's 144 bytes; and 65,536 x 36 bytes
 * through which the host form of sample stages its points a piece at a time. The host forms run on the volume's stream and synchronise; the
 * device forms enqueue on `stream` (NULL = the null stream) and return. Calls on one volume are serialised by the volume: each records an
 * event that the next call's stream waits for. The bake records the scene's per-stream event through rt_trace_paths_device, so
 * rt_scene_update waits for it, and a bake after an update sees the moved geometry. A volume is destroyed before its scene.
 * Refused with RT_ERR_INVALID before any HIP call, in this order: NULL handles or required pointers; a count outside 1 .. 256; a spacing that
 * is not finite or not > 0; an origin that is not finite; max_dirs outside 1 .. 65536; probes * max_dirs >= 2^31; flags other than 0;
 * dirs == 0 or dirs > max_dirs; max_depth == 0; sample or get_sh before any bake or set_sh. After these, rt_probe_volume_create returns
 * RT_ERR_NO_DEVICE for a host-only scene.
 * Limits: the validity flag is the only visibility handling (no depth moments, so light leaks through thin walls between probes); a probe
 * inside a solid is valid and dark, not moved; bands 0 to 2 only, no L1-only table; no windowing against ringing; a bake is whole, not
 * incremental; one device. */
typedef struct rt_probe_volume rt_probe_volume;
typedef struct rt_probe_volume_desc { float origin[3]; float spacing[3]; uint32_t count[3]; uint32_t max_dirs; } rt_probe_volume_desc; /* 40 bytes */
typedef struct rt_probe_bake_params { uint32_t dirs, max_depth, rr_start, seed; } rt_probe_bake_params;                              /* 16 bytes */
typedef struct rt_probe_stats       { uint32_t probes, valid; uint64_t rays; } rt_probe_stats;                                      /* 16 bytes */
int  rt_probe_volume_create(rt_scene* scene, const rt_probe_volume_desc* desc, uint32_t flags, rt_probe_volume** out);
void rt_probe_volume_destroy(rt_probe_volume* vol);
int  rt_probe_volume_entries(rt_probe_volume* vol, const rt_probe_bake_params* p, float* pos, float* dir, uint32_t* state);
int  rt_probe_volume_entries_device(rt_probe_volume* vol, const rt_probe_bake_params* p, void* d_pos, void* d_dir, void* d_state, void* stream);
int  rt_probe_volume_bake(rt_probe_volume* vol, const rt_probe_bake_params* p, float* out_sh, rt_probe_stats* stats);
int  rt_probe_volume_bake_device(rt_probe_volume* vol, const rt_probe_bake_params* p, void* d_out_sh, void* d_stats, void* stream);
int  rt_probe_volume_set_sh(rt_probe_volume* vol, const float* sh);
int  rt_probe_volume_set_sh_device(rt_probe_volume* vol, const void* d_sh, void* stream);
int  rt_probe_volume_get_sh(rt_probe_volume* vol, float* sh);
int  rt_probe_volume_get_sh_device(rt_probe_volume* vol, void* d_sh, void* stream);
int  rt_probe_volume_sample(rt_probe_volume* vol, uint32_t n, const float* pos, const float* normal, float* out_rgb);
int  rt_probe_volume_sample_device(rt_probe_volume* vol, uint32_t n, const void* d_pos, const void* d_normal, void* d_out_rgb, void* stream);

/* ---- Reflection probes: cube-map captures of the arriving radiance at `count` positions of one scene, baked around one path query on one
 * stream, prefiltered into a chain of levels for growing roughness, and sampled along caller-supplied directions: glossy light for what has
 * no parametrisation of its own (moving objects, particles, a rasterised pass that wants the scene's light along a reflection vector). With
 * the lightmap (static diffuse) and the probe volume (dynamic diffuse) this is the third part of the baked-lighting set.
 * Layout. Level l has six faces of S_l = size >> l texels on an edge. A probe's chain is its levels in order, l = 0 .. levels-1; within a
 * level the faces run 0 to 5, then y, then x: texel ((f * S_l) + y) * S_l + x. One float4 per texel: rgb in .xyz and the probe's validity in
 * .w, 1.0f or 0.0f. Probes are consecutive: probe p's chain starts at float4 p * C, C = the sum of 6 * S_l * S_l over the levels.
 * Face f at face coordinates (s, t) in [-1, 1]^2 has the unnormalised direction
 *     0 (+x): ( 1, -t, -s)     1 (-x): (-1, -t,  s)     2 (+y): ( s,  1,  t)     3 (-y): ( s, -1, -t)     4 (+z): ( s, -t,  1)     5 (-z): (-s, -t, -1)
 * and texel (x, y) of level l has its centre at s = ((float)x + 0.5f) * (2.0f / (float)S_l) - 1.0f, t likewise from y.
 * Every operation below is one R1 fp32 operation of DESIGN.md §3, left to right as bracketed, never contracted; sqrt and the divisions are
 * correctly rounded; dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; there is no transcendental function. next(a) is the renderers'
 * xorshift32 draw. unit(v): i = 1.0f / sqrt(dot(v, v)) (two roundings), the direction v * i and the weight (i * i) * i, with v the face
 * direction as the table above writes it (its component order is the dot's).
 *   1. Entries. T = ((p * 6 + f) * size + y) * size + x is the global index of a level-0 texel; texel T and sample j make entry
 *      e = T * spt + j with the state a = (seed + (e + 1) * 0x9E3779B9) mod 2^32, 0 replaced by 0x9E3779B9 (the lightmap's rule).
 *      u1 = next(a), u2 = next(a); s = ((float)x + u1) * (2.0f / (float)size) - 1.0f, t likewise from y and u2. org = the probe's position,
 *      dir = face f's direction at (s, t), unnormalised (the path query stores its own half copy); the entry's path state is a after the
 *      two draws.
 *   2. Paths. One rt_trace_paths_device over the count * 6 * size^2 * spt entries: samples = 1, max_depth and rr_start as given, rng_out
 *      NULL, rays kept. A probe outside the contract range is rejected there, all its entries together; it is then INVALID: every texel of
 *      every level is four zeros.
 *   3. Resolve, per level-0 texel of a valid probe and per channel: C = +0; for j = 0 .. spt-1 in order, C = C + r, r the entry's radiance,
 *      replaced by fminf(r, clamp) first when clamp > 0; texel = C / (float)spt, .w = 1.
 *   4. Prefilter, for l = 1 .. levels-1 and every texel of level l of a valid probe. n = unit(the output texel's centre direction)'s
 *      direction. The table holds, per level-0 texel k in layout order, (d_k, o_k) = unit(its centre direction): o_k is the texel's solid
 *      angle up to a constant that cancels. q_l = 2 * (levels - l) - 1 squarings: the lobe is cos^(2^q_l), from cos^2 at the last level
 *      to cos^(2^(2 * levels - 3)) at level 1. W = A = +0; for k = 0 .. 6 * size^2 - 1 in order: c = dot(n, d_k); a term with !(c > 0) is
 *      skipped (by a select: it multiplies nothing, so a non-finite texel behind the lobe does not reach the sum); otherwise c is squared q_l
 *      times (c = c * c), w = c * o_k, W = W + w, and per channel A = A + w * texel_k. out = A / W, .w = 1. The sum is one lane's, in layout
 *      order, with no cross-lane reduction and no atomics. Every level is made from level 0, not from the level below. The table depends
 *      on size alone and is built once, at creation, by a kernel in this arithmetic.
 *   5. Stats: probes, valid, and rays = the sum of the entries' ray counts over the valid probes. d_stats holds the same 16 bytes.
 *   6. Sample, per point: a probe index, a position (optional), a direction r (any length) and a level of detail lod.
 *      Invalid inputs: probe_index >= count, a non-finite component of pos, r or lod, and a lookup direction (below) whose largest
 *      |component| is 0 or that is not finite, each give three NaNs. Otherwise an invalid probe gives (0, 0, 0).
 *      Parallax box, when the probes were created with boxes and pos is not NULL: per axis a, t_a = ((r_a > 0 ? max_a : min_a) - pos_a) / r_a,
 *      or +inf when r_a == 0; t = fminf(fminf(t_x, t_y), t_z). If t > 0 and finite, the lookup direction is L_a = (pos_a + r_a * t) -
 *      centre_a, the point where the ray leaves the box seen from the probe; otherwise L = r, as it is without a box or without pos.
 *      Face: the major axis is the largest |L_a|, ties to x, then y (x if |L_x| >= |L_y| and |L_x| >= |L_z|, else y if |L_y| >= |L_z|); m is
 *      that |component|, the face the axis' by the component's sign, and (s, t) the inverse of the table, each one division by m:
 *      0: (-L_z / m, -L_y / m)   1: (L_z / m, -L_y / m)   2: (L_x / m, L_z / m)   3: (L_x / m, -L_z / m)   4: (L_x / m, -L_y / m)   5: (-L_x / m, -L_y / m).
 *      Levels: lod = fminf(fmaxf(lod, 0.0f), (float)(levels - 1)); l0 = min((int)lod, levels - 2); fl = lod - (float)l0.
 *      Per level, bilinear inside the face: fx = (s + 1.0f) * (0.5f * (float)S_l) - 0.5f, clamped to [0, S_l - 1] (fminf(fmaxf(..)));
 *      x0 = min((int)fx, S_l - 2); g = fx - (float)x0; the weights are wx = (1.0f - g, g); y likewise from t. V = +0; over the taps
 *      (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) in this order, V = V + (wy * wx) * texel per channel. Nothing is filtered
 *      across face edges. out = a * (1.0f - fl) + b * fl, a and b the values of levels l0 and l0 + 1; with levels == 1, out = a.
 * Radiance is linear and nothing multiplies by a material: the specular colour x result is the caller's.
 * rt_reflection_probes_entries[_device] return step 1: pos, dir (3 floats per entry each) and state (a word per entry) for
 * count * 6 * size^2 * spt entries; any may be NULL, not all three. rt_reflection_probes_bake[_device] run steps 1 to 5; the chain stays in
 * the object, and out_chain (count * C * 4 floats; the device pointer 16-byte aligned) receives a copy when it is not NULL; stats / d_stats
 * may be NULL. rt_reflection_probes_set_level0[_device] load level 0 of every probe (count * 6 * size^2 * 4 floats, probes consecutive; a
 * synthetic capture or a saved one; .w of a probe's first texel is its validity): the levels above become STALE.
 * rt_reflection_probes_prefilter[_device] run step 4 alone on the level 0 held (an invalid probe's higher levels become zeros).
 * rt_reflection_probes_get_chain[_device] copy the whole chain out. rt_reflection_probes_sample[_device] run step 6 on n points:
 * probe_index n words, pos 3n floats or NULL, dir 3n floats, lod n floats, out_rgb 3n floats; n == 0 is RT_OK with nothing launched.
 * The object owns every device buffer it needs, allocated by rt_reflection_probes_create: no later call allocates. Per entry, max_spt of
 * them per level-0 texel: pos, dir, state, radiance and ray count (12 + 12 + 4 + 12 + 4 = 44 bytes); per chain texel 16 bytes; the table's
 * 6 * size^2 float4; the positions and boxes (36 bytes per probe); and 65,536 x 44 bytes through which the host form of sample stages its
 * points a piece at a time. pos (3 * count floats) and box (NULL, or 6 * count floats, min then max per probe) are copied at creation. The
 * host forms run on the object's stream and synchronise; the device forms enqueue on `stream` (NULL = the null stream) and return. Calls on
 * one object are serialised by the object: each records an event that the next call's stream waits for. The bake records the scene's
 * per-stream event through rt_trace_paths_device, so rt_scene_update waits for it, and a bake after an update sees the moved geometry. The
 * object is destroyed before its scene.
 * Refused with RT_ERR_INVALID before any HIP call, in this order: NULL handles or required pointers; count outside 1 .. 4096; size not a
 * power of two in 8 .. 128; levels outside 1 .. log2(size) - 1 (the smallest face is 4); max_spt outside 1 .. 1024;
 * count * 6 * size^2 * max_spt >= 2^31; a position or box value that is not finite, or a box with min > max; flags other than 0; spt == 0 or
 * spt > max_spt; max_depth == 0; a clamp that is NaN or negative; prefilter, get_chain or sample before any bake or set_level0; sample with
 * stale levels (after set_level0 without a prefilter, when levels > 1). After these, rt_reflection_probes_create returns RT_ERR_NO_DEVICE for
 * a host-only scene.
 * Limits: no filtering across cube-face edges (a seam shows at high roughness); a cosine-power lobe about the lookup direction, no GGX and
 * no importance sampling; the caller chooses and blends probes per point; probes do not move after creation; a bake is whole (every entry
 * at once, not in batches; not incremental); fp32 storage; one device. */
typedef struct rt_reflection_probes rt_reflection_probes;
typedef struct rt_reflection_probes_desc {
    uint32_t count, size, levels, max_spt;
    const float* pos;       /* 3 * count                                                       */
    const float* box;       /* NULL, or 6 * count: min then max per probe                      */
} rt_reflection_probes_desc;                                                                                                        /* 32 bytes */
typedef struct rt_reflection_bake_params { uint32_t spt, max_depth, rr_start, seed; float clamp; } rt_reflection_bake_params;        /* 20 bytes */
typedef struct rt_reflection_stats       { uint32_t probes, valid; uint64_t rays; } rt_reflection_stats;                            /* 16 bytes */
int  rt_reflection_probes_create(rt_scene* scene, const rt_reflection_probes_desc* desc, uint32_t flags, rt_reflection_probes** out);
void rt_reflection_probes_destroy(rt_reflection_probes* probes);
int  rt_reflection_probes_entries(rt_reflection_probes* probes, const rt_reflection_bake_params* p, float* pos, float* dir, uint32_t* state);
int  rt_reflection_probes_entries_device(rt_reflection_probes* probes, const rt_reflection_bake_params* p, void* d_pos, void* d_dir, void* d_state,
                                         void* stream);
int  rt_reflection_probes_bake(rt_reflection_probes* probes, const rt_reflection_bake_params* p, float* out_chain, rt_reflection_stats* stats);
int  rt_reflection_probes_bake_device(rt_reflection_probes* probes, const rt_reflection_bake_params* p, void* d_out_chain, void* d_stats, void* stream);
int  rt_reflection_probes_set_level0(rt_reflection_probes* probes, const float* level0);
int  rt_reflection_probes_set_level0_device(rt_reflection_probes* probes, const void* d_level0, void* stream);
int  rt_reflection_probes_prefilter(rt_reflection_probes* probes);
int  rt_reflection_probes_prefilter_device(rt_reflection_probes* probes, void* stream);
int  rt_reflection_probes_get_chain(rt_reflection_probes* probes, float* chain);
int  rt_reflection_probes_get_chain_device(rt_reflection_probes* probes, void* d_chain, void* stream);
int  rt_reflection_probes_sample(rt_reflection_probes* probes, uint32_t n, const uint32_t* probe_index, const float* pos, const float* dir,
                                 const float* lod, float* out_rgb);
int  rt_reflection_probes_sample_device(rt_reflection_probes* probes, uint32_t n, const void* d_probe_index, const void* d_pos, const void* d_dir,
                                        const void* d_lod, void* d_out_rgb, void* stream);

/* ---- Renderers: == IRenderer implementations (src/render.hpp:11-18) ------------------------ */
enum {
    RT_RENDERER_MEGAKERNEL = 0, /* MegakernelRenderer (src/render_megakernel.hpp:13-19) */
    RT_RENDERER_WAVEFRONT = 1   /* WavefrontRenderer  (src/render_wavefront.hpp:55-61)  */
};
/* Per-pixel xorshift seed:
 *   RT_SEED_WAVEFRONT : x + y*W                        (src/render_wavefront.cpp:69-73)
 *   RT_SEED_MEGAKERNEL: x*H8 + y, H8 = 8*ceil(H/8)     (src/render_megakernel.cpp:90-93,144-146)
 *   RT_SEED_DEFAULT   : the renderer kind's own rule */
enum { RT_SEED_DEFAULT = 0, RT_SEED_WAVEFRONT = 1, RT_SEED_MEGAKERNEL = 2 };

/* == the renderer constructors (App&, img_size, image&, max_depth, sample_count). The output
 * image is passed to rt_render_frame instead of being captured by reference. */
int rt_renderer_create(int kind, rt_scene* scene, int32_t width, int32_t height,
                       uint32_t max_depth, uint32_t sample_count, uint32_t seed_mode,
                       rt_renderer** out);
void rt_renderer_destroy(rt_renderer* r);

/* Multi-GPU tile split (no reference counterpart: the reference is single-device). The frame is
 * cut into horizontal strips of `strip_rows` rows; strip k belongs to rank k % world. A renderer
 * renders only its own strips, packed top to bottom into a compact buffer of
 * rt_renderer_local_rows() rows. RNG seeds use GLOBAL pixel coordinates, so the union of the
 * tiles is bit-identical to a single-GPU frame. Default: rank 0 of world 1. */
int rt_renderer_set_tile(rt_renderer* r, uint32_t rank, uint32_t world, uint32_t strip_rows);
int32_t rt_renderer_local_rows(const rt_renderer* r);
/* Global row index of local row `local_row` (for de-interleaving a gathered frame). */
int32_t rt_renderer_global_row(const rt_renderer* r, int32_t local_row);

/* Per-launch hipEvent timing of the traversal / shading kernels, each on the stream it is launched on: rt_stats.hot_kernel_ms (the
 * dominant kernel of the schedule that ran: k_megakernel, k_wf_finish, k_wf_extend or the fused per-bounce kernel) and
 * rt_stats.kernel_ms[RT_K_*] per family. The megakernel is always timed; off by default for the wavefront renderer (two event records per
 * launch — three per EXTEND + SHADE pair —, which the per-bounce schedules with their thousands of launches per frame feel); also enabled
 * by the environment variable RT_PROFILE_KERNELS=1 at renderer creation. No reference counterpart (the reference's print_elapsed helper is
 * commented out: src/render_wavefront.cpp:129-137). */
int rt_renderer_set_profiling(rt_renderer* r, int enable);

/* Russian roulette, an EXTENSION: the reference only lists it as a to-do (PLAN.md:23-27) and never implements
 * it, so it is off by default (start_bounce = 0) and changes the image and the ray count when turned on.
 * A path that continues after its bounce b, start_bounce <= b < max_depth, survives with probability
 * p = clamp(max component of its stored attenuation, 0.05, 1) (one extra RNG draw) and carries on with
 * attenuation / p; otherwise it ends with no contribution. Same rule in both renderers and in the oracle. */
int rt_renderer_set_russian_roulette(rt_renderer* r, uint32_t start_bounce);

/* Per-frame seed salt (no reference counterpart: the reference seeds a pixel from its coordinates alone, so every frame of an animation carries
 * the same noise). A pixel's xorshift chain starts at pixel_seed(x, gy, W, H, seed_mode) + salt * 0x9E3779B9u (uint32, wrapping); salt 0, the
 * default, is the reference's seed: the same frames bit for bit. It holds for the frames begun after the call, under both renderers and every
 * schedule, slicing and tile split (seeds stay a function of GLOBAL pixel coordinates: tiles still union to the single-GPU frame). A continuation
 * (rt_render_frame_continue*) goes on with the chain it was started with, whatever the salt is by then. RT_ERR_INVALID while a frame is in
 * flight; a captured hipGraph is re-captured by the next frame when the salt changed. An animation passes its frame number. */
int rt_renderer_set_frame_seed(rt_renderer* r, uint32_t salt);

/* ---- Schedule of the wavefront renderer --------------------------------------------------------------------------------
 * The reference's WavefrontRenderer::render_frame (src/render_wavefront.cpp:396-431) has ONE schedule: per sample, one
 * generate_camera_rays launch and one shoot_rays launch per bounce, survivors compacted between bounces (:282-311). This
 * library renders the same frame (bit for bit) under several schedules; which one runs is chosen here — never silently — and
 * reported back in rt_stats, per kernel family, so that a test can assert that the kernels it means to test were launched.
 *   finish_depth        bounces rendered launch by launch: k_wf_extend + k_wf_shade with __ballot / mbcnt compaction of the
 *                       survivors into the next queue, the reference's shape. The rest of every path is followed by
 *                       k_wf_finish in one launch. 0 = everything in k_wf_finish (default); RT_SCHED_ALL_BOUNCES (or any
 *                       value >= max_depth) = the reference's per-bounce schedule.
 *   samples_per_launch  samples of a pixel one k_wf_finish launch renders. 0 = all of them: ONE launch per frame (default).
 *   stream_lanes        interleaved sub-tiles rendered on HIP streams of their own. 0 = automatic (1 for the one-launch
 *                       schedule, 3 for a launch or launch pair per bounce all the way down, 2 otherwise). HIP serves streams from
 *                       GPU_MAX_HW_QUEUES hardware queues (default 4). The library never changes the environment: a HOST may set the
 *                       variable before its first HIP call; the library reads it once, when the process's first renderer is
 *                       created, and resolves an automatic lane count down to lanes + 2 <= queues (rt_stats.hw_queues / .stream_lanes).
 *                       Renderers of one device share their lane streams: drive them from one host thread.
 *   requeue             with samples_per_launch > 1: 1 = a pixel between two samples goes through a device-wide dynamic queue
 *                       (breadth first), 0 = it stays in its lane (depth first), -1 = automatic.
 *   reorder, matsort    SURVEY 8(f) row f-3, per-bounce schedule only: k_wf_shade bins a block's survivors by direction octant
 *                       and 4x4x4 origin cell / partitions a block's rays by material kind before shading.
 *   cost_order          one-launch schedule: sample 0 in a launch of its own, the other samples with the most expensive 8x8
 *                       blocks first. -1 = automatic (>= 32 spp, 1..4 pixel generations), 0 = off, 1 = whenever the tile
 *                       consists of whole 8x8 blocks (a tile that does not falls back to queue order).
 *   hip_graph           1 = the frame's launches are captured once and replayed as a hipGraph.
 *   fused_bounce        1 = the bounces rendered launch by launch (finish_depth) use ONE kernel per bounce that intersects, shades and
 *                       compacts the survivors into the next queue — shoot_rays as the reference has it (src/render_wavefront.cpp:222-312)
 *                       — instead of the EXTEND + SHADE pair with its hit-record round trip. reorder / matsort act in k_wf_shade and
 *                       are ignored then.
 *   pixel_slices        Both renderers (the only field MEGAKERNEL renderers use). A pixel's samples are a sequential chain (one RNG
 *                       word), but not bound to one lane: the chain is cut into slices of decreasing length, all first slices are
 *                       rendered, then all second ones ..., the pixel's colour sum and RNG word travelling through memory in between, so
 *                       that the frame drains over its last, short slices instead of over whole pixels (bit-identical frame). -1 =
 *                       automatic (as many as the tile's size calls for; one for a tile of at most ~1.25 pixels per resident lane), 0 or
 *                       1 = off, 2 .. 8 = that many, whatever the tile's size (at most one slice per sample; above 64 samples per unit of
 *                       2, 4, ... samples). The wavefront renderer slices its one-launch schedule (samples_per_launch 0, finish_depth 0)
 *                       only, and not with hip_graph, more than one stream lane, or cost_order = 1. rt_stats.pixel_slices reports what
 *                       ran.
 * Environment: the library reads GPU_MAX_HW_QUEUES (above), RT_PROFILE_KERNELS=1 (rt_renderer_set_profiling at creation) and
 * RT_KERNEL_STATS=1 (the instrumented kernel instantiations; their report goes to stderr) — and nothing else. Sweep knobs and test
 * hooks (RT_WF_*, RT_MEGA_*, RT_BVH_*, RT_INJECT_ALLOC_FAILURE) exist in the developer build only: `make -C csrc dev` ->
 * librt_mi355x_dev.so (csrc/rt_knobs.h). */
#define RT_SCHED_ALL_BOUNCES 0xFFFFFFFFu
typedef struct rt_schedule {
    uint32_t finish_depth;
    uint32_t samples_per_launch;
    uint32_t stream_lanes;
    int32_t requeue;
    uint32_t reorder;
    uint32_t matsort;
    int32_t cost_order;
    uint32_t hip_graph;
    uint32_t fused_bounce;
    int32_t pixel_slices; /* (ABI 8) both renderers (the wavefront renderer's one-launch schedule) */
} rt_schedule;
/* Megakernel renderers accept the call and use pixel_slices only. No frame may be in flight; the tile's queues are re-allocated. */
int rt_renderer_set_schedule(rt_renderer* r, const rt_schedule* s);
int rt_renderer_get_schedule(const rt_renderer* r, rt_schedule* out);

/* Kernel families, for rt_stats::launches_by_kernel. A k_wf_shade launch counts in RT_K_WF_SHADE and, when the flags are on,
 * also in RT_K_WF_SHADE_REORDER / RT_K_WF_SHADE_MATSORT; a k_wf_finish launch with the dynamic queue counts in RT_K_WF_FINISH
 * and RT_K_WF_FINISH_REQUEUE. */
enum {
    RT_K_MEGAKERNEL = 0,
    RT_K_WF_INIT = 1,
    RT_K_WF_GENERATE = 2,
    RT_K_WF_EXTEND = 3,
    RT_K_WF_SHADE = 4,
    RT_K_WF_SHADE_REORDER = 5,
    RT_K_WF_SHADE_MATSORT = 6,
    RT_K_WF_FINISH = 7,
    RT_K_WF_FINISH_REQUEUE = 8,
    RT_K_WF_TILE_ORDER = 9, /* k_wf_tile_cost + k_wf_order_tiles (cost ordering) */
    RT_K_WF_RESOLVE = 10,
    RT_K_FILL_BLACK = 11,
    RT_K_WF_SHOOT = 12, /* k_wf_finish limited to one bounce: intersect + shade + compact, one launch per bounce (fused_bounce) */
    RT_K_BLOCK_RESOLVE = 13, /* k_blocks_resolve: the megakernel's whole image of a block continuation (adaptive sampling) */
    RT_K_COUNT = 16
};

typedef struct rt_stats {
    uint64_t rays;       /* trace_ray calls (src/render_megakernel.cpp:32, render_wavefront.cpp:407) */
    double seconds;      /* host wall clock, first launch -> last kernel complete                  */
    double device_ms;    /* same region measured with hipEvents on the render stream               */
    double hot_kernel_ms;/* summed duration of the dominant kernel's launches (hipEvents), or 0    */
    uint32_t hot_kernel_launches;
    uint32_t launches;   /* kernel launches issued for the frame                                   */
    /* what actually ran (ABI 5): launches of the frame per kernel family, and the schedule as it was resolved for this tile */
    uint32_t launches_by_kernel[RT_K_COUNT];
    uint32_t stream_lanes;       /* HIP streams the frame's launch chains ran on (1 for the megakernel)            */
    uint32_t samples_per_launch; /* samples of a pixel per k_wf_finish launch as resolved (spp = one launch per frame) */
    uint32_t finish_depth;       /* bounces rendered as EXTEND + SHADE launch pairs, min(schedule, max_depth)      */
    uint32_t cost_ordered;       /* 1 = the cost-ordered second launch ran                                          */
    /* with profiling on (rt_renderer_set_profiling): summed hipEvent duration of the launches of the traversal / shading kernel
     * families (RT_K_MEGAKERNEL, RT_K_WF_EXTEND, RT_K_WF_SHADE, RT_K_WF_SHOOT, RT_K_WF_FINISH), each on the stream it was launched on; else 0 */
    double kernel_ms[RT_K_COUNT];
    /* (ABI 7) hardware queues the library assumed HIP serves the process's streams from: GPU_MAX_HW_QUEUES as the HOST had set it when the
     * renderer was created, 4 (HIP's default) when unset. The library never changes the environment; an automatic stream-lane count is resolved
     * down to lanes + 2 <= hw_queues (the frame's stream and one stream of the host framework beside the lanes'), see stream_lanes above. */
    uint32_t hw_queues;
    uint32_t pixel_slices; /* (ABI 8) slices a pixel's samples were rendered in (1 = every pixel on one lane, an empty tile, an unsliced schedule) */
} rt_stats;

/* == IRenderer::render_frame(camera, scene) (src/render_megakernel.cpp:75-187,
 * src/render_wavefront.cpp:396-431). Renders this renderer's tile and copies it to host:
 *   rgba_f32: local_rows*W*4 floats, the pre-quantisation framebuffer (sqrt(mean rgb), alpha 1)
 *   rgba_u8 : local_rows*W*4 bytes, what the reference's RGBA-unorm8 image holds
 * Either may be NULL. Unlike the reference it prints nothing and writes no file: the caller
 * (host adapter / CLI) prints the three stat lines and writes out.png. */
int rt_render_frame(rt_renderer* r, const rt_camera* cam, float* rgba_f32, uint8_t* rgba_u8,
                    rt_stats* stats);

/* Same, but the outputs are DEVICE pointers on the renderer's device (e.g. a tensor's data_ptr)
 * and `stream` is a hipStream_t (NULL = the renderer's own stream). Returns after the frame has
 * completed on the device (stats need the ray counter). */
int rt_render_frame_device(rt_renderer* r, const rt_camera* cam, void* d_rgba_f32,
                           void* d_rgba_u8, void* stream, rt_stats* stats);

/* The same frame in two calls: _begin enqueues it on `stream` (NULL = the renderer's own) and returns at once, _end waits
 * for it and fills `stats`. One frame per renderer may be in flight; frames of DIFFERENT renderers overlap on the device,
 * which is how a caller hides the end-of-frame drain (the last pixels' sequential samples) behind the next frame.
 * No reference counterpart (the reference blocks after every kernel: src/render_wavefront.cpp:396-431). */
int rt_render_frame_begin(rt_renderer* r, const rt_camera* cam, void* d_rgba_f32, void* d_rgba_u8, void* stream);
int rt_render_frame_end(rt_renderer* r, rt_stats* stats);

/* ---- Progressive rendering (no reference counterpart: the reference renders every frame from scratch, src/main.cpp:57-70).
 * A pixel's samples are one sequential chain: one xorshift word and three fp32 sums, added in sample order. With progressive rendering
 * on, every frame (rt_render_frame, _device, _begin + _end) also stores each pixel's final sums and RNG word, 16 bytes per pixel of the
 * tile, and its output is unchanged. rt_render_frame_continue[_device] then adds `samples` samples to every pixel of the last frame, with
 * that frame's camera, starting from the stored state, and writes sqrt(sum / total) as fp32 and unorm8 exactly as a frame does, total =
 * the pixel's samples in all. The identity this guarantees: a frame of a samples followed by continuations of b1, b2, ... samples gives,
 * bit for bit in both images and in the summed ray counts, the frame of a + b1 + b2 + ... samples — under every schedule a frame
 * accepts, and for the strips of a multi-GPU split (rt_frame_gather after a host continuation gathers the accumulated image).
 * rt_stats describes the call alone (its rays, launches, slices: a continuation of b samples is planned as a frame of b samples).
 *   rt_renderer_set_progressive(r, 1) allocates the state, (r, 0) frees it; no frame may be in flight.
 *   rt_render_frame_continue[_device] returns RT_ERR_INVALID when progressive rendering is off, when no frame has completed since it was
 *   turned on or since the state was discarded, for samples == 0, and when the total would exceed 2^24 (past which (float)total is not
 *   exact); RT_ERR_UNSUPPORTED under rt_schedule::hip_graph = 1. rt_renderer_set_tile, rt_renderer_set_schedule,
 *   rt_renderer_set_russian_roulette and rt_renderer_set_progressive discard the state.
 *   rt_renderer_accumulated_samples: the samples the stored state holds (0: nothing to continue). */
int rt_renderer_set_progressive(rt_renderer* r, int enable);
int rt_render_frame_continue(rt_renderer* r, uint32_t samples, float* rgba_f32, uint8_t* rgba_u8, rt_stats* stats);
int rt_render_frame_continue_device(rt_renderer* r, uint32_t samples, void* d_rgba_f32, void* d_rgba_u8,
                                    void* stream, rt_stats* stats);
int rt_renderer_accumulated_samples(const rt_renderer* r, uint32_t* out);

/* ---- Adaptive sampling (no reference counterpart): continue a progressive frame only where it is still noisy.
 * A BLOCK is an 8x8 pixel block of the renderer's tile: rt_renderer_block_grid gives blocks_x = ceil(width / 8) per row and blocks_y =
 * ceil(local_rows / 8) rows; block b covers columns (b % blocks_x) * 8 ... + 7 and tile rows (b / blocks_x) * 8 ... + 7 (the tile's rows as
 * rt_frame_gather lays them out, tile-local), as far as they lie in the image. Progressive rendering keeps, beside every pixel's chain state, a
 * sample count per block: a frame sets every block to its spp, a continuation adds `samples` to every block, a block continuation to the blocks it
 * lists. A pixel's chain is its own, so the identity of progressive rendering holds per pixel: every pixel whose block holds n samples is, bit
 * for bit in both images, the pixel of a frame of n samples, and the rays of the calls sum to those of the frames of the blocks' totals.
 * rt_renderer_accumulated_samples returns the SMALLEST block count (0: nothing to continue); rt_render_frame_continue stays valid after block
 * continuations (every block gains `samples`).
 *   rt_render_frame_continue_blocks[_device] renders `samples` more samples for the pixels of the n_blocks listed blocks (host memory, both
 *   variants; any order, no index twice) and writes the tile's WHOLE current image: every other pixel gets sqrt(sum / its block's count) and its
 *   unorm8, as a frame would. n_blocks == 0 traces nothing and writes the current image. RT_ERR_INVALID for an index out of range or listed
 *   twice, samples == 0, a listed block whose count would exceed 2^24, and wherever rt_render_frame_continue refuses; RT_ERR_UNSUPPORTED under
 *   hip_graph = 1, and on the wavefront renderer for every schedule but its one-launch default (finish_depth 0, samples_per_launch 0; with
 *   max_depth 0 every schedule). rt_stats describes the call: its rays, launches and slices.
 *   rt_renderer_block_samples: the blocks' counts, blocks_x * blocks_y of them in host memory (zeros when there is nothing to continue).
 * Every call that renders a block first keeps a SNAPSHOT of it: its pixels' sums and its count as they were (16 bytes per pixel, 4 per block);
 * a frame clears the snapshots. The policy compares a block with its snapshot (Dammertz et al., "A Hierarchical Automatic Stopping Condition for
 * Monte Carlo Global Illumination", 2009: the two-image criterion, with "A" = the block as of its previous render). For a block B with count n and
 * snapshot count n' (n' < n), for each pixel p of B that lies in the image:
 *   I_p = sum_p / n, in linear RGB;
 *   A_p = snapshot sum_p / n';
 *   e_p = (|I_r - A_r| + |I_g - A_g| + |I_b - A_b|) / sqrt(eps + I_r + I_g + I_b), eps = 1e-4;
 *   e_B = the mean of e_p over B's pixels that lie in the image.
 * With b = n' (a doubling schedule) A holds exactly half of I's samples, the published setting. A block is ACTIVE when it has no snapshot yet
 * (n' = 0: the first call after a frame), when n < min_samples, or when e_B >= threshold.
 *   rt_renderer_adapt evaluates every block and writes the active ones, ascending, to blocks_out (room for blocks_x * blocks_y) and their number
 *   to n_out; it renders nothing. rt_renderer_block_errors: the last evaluation's e_B per block (+inf where n' = 0; zeros before the first).
 *   rt_render_frame_continue_adaptive[_device] evaluates, continues the active blocks by `samples` (as rt_render_frame_continue_blocks, whose
 *   refusals it shares) and reports their number in n_blocks_out (may be null). It reads the list back to the host on the way: one small sync. */
int rt_renderer_block_grid(const rt_renderer* r, uint32_t* blocks_x, uint32_t* blocks_y);
int rt_render_frame_continue_blocks(rt_renderer* r, uint32_t samples, const uint32_t* blocks, uint32_t n_blocks,
                                    float* rgba_f32, uint8_t* rgba_u8, rt_stats* stats);
int rt_render_frame_continue_blocks_device(rt_renderer* r, uint32_t samples, const uint32_t* blocks, uint32_t n_blocks,
                                           void* d_rgba_f32, void* d_rgba_u8, void* stream, rt_stats* stats);
int rt_renderer_block_samples(const rt_renderer* r, uint32_t* out);
int rt_renderer_adapt(rt_renderer* r, float threshold, uint32_t min_samples, uint32_t* blocks_out, uint32_t* n_out);
int rt_render_frame_continue_adaptive(rt_renderer* r, uint32_t samples, float threshold, uint32_t min_samples,
                                      float* rgba_f32, uint8_t* rgba_u8, rt_stats* stats, uint32_t* n_blocks_out);
int rt_render_frame_continue_adaptive_device(rt_renderer* r, uint32_t samples, float threshold, uint32_t min_samples,
                                             void* d_rgba_f32, void* d_rgba_u8, void* stream, rt_stats* stats,
                                             uint32_t* n_blocks_out);
int rt_renderer_block_errors(const rt_renderer* r, float* out);

/* ---- Primary-hit G-buffer and the a-trous denoiser (no reference counterpart: the reference returns the raw Monte Carlo estimate).
 *
 * rt_scene_gbuffer: the guide images of a camera's first hits, one unjittered ray per pixel. H = cam->height rows, W = cam->width columns,
 * row 0 first; each output is H*W*4 fp32. Per pixel (x, y), in R1 arithmetic:
 *   pc = (pixel00 + (float)x * delta_u) + (float)y * delta_v (camera_ray's pixel centre, no jitter); d = pc - center (fp32, not half);
 *   org = center. The hit is rt_intersect_batch's closest hit of (org, d): t, u, v and the triangle are its, bit for bit.
 *   miss: albedo = (sky, 0), normal = (0, 0, 0, 0), position = (0, 0, 0, +inf)
 *   hit:  w, tu, tv, the interpolated normal and the world-space shading normal with exactly the expressions of shading (rt_device.h:
 *         shade_hit): normals and uvs of the triangle's shading record, its instance's normal matrix, both normalisations normalize3.
 *         albedo = the attenuation the first bounce's scatter applies, alpha 0: diffuse and metallic the material's colour or texel
 *         (unorm8_to_float), dielectric (1, 1, 1), RT_MAT_NONE (0, 0, 0); emission is not included.
 *         normal = (shading normal, 0); position = (org.x + d.x * t, org.y + d.y * t, org.z + d.z * t, t).
 * The G-buffer belongs to the scene, not to a renderer: every full-frame rendering of cam shares it, whatever the tile split (a multi-GPU
 * frame: the root device's scene computes the G-buffer of the gathered frame). Refused: RT_ERR_INVALID for a NULL argument, width or
 * height <= 0, or a camera centre outside the contract range (rt_render_frame*'s check); RT_ERR_NO_DEVICE for a host-only scene.
 * The host variant synchronises. The _device variant enqueues on `stream` (NULL = the null stream) and returns; the scene records an event
 * behind the launch, one event per stream used, and rt_scene_update waits for all of them before it writes: launches pending on any number of
 * streams read the scene as it was, and the update stays synchronous. */
int rt_scene_gbuffer(rt_scene* scene, const rt_camera* cam, float* albedo, float* normal, float* position);
int rt_scene_gbuffer_device(rt_scene* scene, const rt_camera* cam, void* d_albedo, void* d_normal, void* d_position, void* stream);

/* The motion guide: rt_scene_gbuffer (the same three planes, bit for bit) plus a fourth H x W x 4 plane from the same traversal, where each
 * visible surface point was before the scene's last update. For a hit on triangle T (rt_intersect_batch's index: a pre-split triangle reports its
 * original) at (u, v), with T's PREVIOUS world-space vertices b0, b1, b2 (RT_SCENE_KEEP_PREVIOUS) and w = (1 - u) - v, per component
 *   prev = (b0 * w + b1 * u) + b2 * v,  prev.w = 1;     a miss writes (0, 0, 0, 0).
 * It covers instance motion and vertex animation alike, and a static scene under a moving camera (create the scene with both flags and never
 * update it: prev_position == position up to the rounding of the two expressions). Refusals as rt_scene_gbuffer, plus RT_ERR_INVALID for a scene
 * created without RT_SCENE_KEEP_PREVIOUS. The _device form records the scene's per-stream event as rt_scene_gbuffer_device does: an update
 * waits for it. */
int rt_scene_gbuffer_motion(rt_scene* scene, const rt_camera* cam, float* albedo, float* normal, float* position, float* prev_position);
int rt_scene_gbuffer_motion_device(rt_scene* scene, const rt_camera* cam, void* d_albedo, void* d_normal, void* d_position,
                                   void* d_prev_position, void* stream);

/* Edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) guided by rt_scene_gbuffer's planes.
 * Inputs are H x W x 4 fp32: the frame as a renderer writes it (rgb = sqrt(mean), alpha 1) and the three guides. Outputs: out_f32 H*W*4
 * floats, out_u8 H*W*4 bytes; either may be NULL, not both. out_f32 may alias rgba_f32 (in-place); no other aliasing is allowed.
 * The filter, every operation one R1 fp32 op, left to right:
 *   1. L_p = (F_r*F_r, F_g*F_g, F_b*F_b): filtering happens in linear radiance.
 *   2. For i = 0 .. iterations-1, step s = 2^i, every pixel p = (x, y): taps q = (x + s*dx, y + s*dy), dy = -2..2 (outer), dx = -2..2
 *      (inner); taps outside the image are skipped, and so is a tap that differs from p in being a hit (a hit: P.w finite).
 *        E = ((dot(L_p-L_q)*kc_i + dot(N_p-N_q)*kn_i) + dot(P_p.xyz-P_q.xyz)*kx) + dot(A_p-A_q)*ka
 *      dot = (x*x + y*y) + z*z; a term whose coefficient is 0 is left out (E starts at +0); k = RN(1/RN(sigma*sigma)), 0 for sigma = +inf;
 *      kc_i = ldexp(kc, 2i) (the colour sigma halves per iteration), kn_i = ldexp(kn, -2i) (the normal distance over the step squared).
 *        w = (h[dy+2]*h[dx+2]) * exp_m(-E), h = {1/16, 1/4, 3/8, 1/4, 1/16}; S += w*L_q per channel, Wsum += w, in tap order
 *        L'_p = S / Wsum (Wsum >= 9/64: the centre tap has E = 0 and exp_m(-0) = 1). L' is the next iteration's L; the guides stay fixed.
 *      exp_m: csrc/denoise_math.h (R1 operations only; within 4 ulp of exp on [-87, 0], exp_m(+-0) = 1, 0 below -87).
 *   3. Output rgb = sqrt(L'), alpha 1; the unorm8 image is to_unorm8 of it, alpha 255, as a frame's.
 *   4. iterations = 0: out_f32 is the frame bit for bit, out_u8 the frame's own unorm8 image.
 * Refused with RT_ERR_INVALID, before any HIP call: NULL handles or pointers, device < 0, non-positive sizes, W * H >= 2^31, a shape so
 * narrow and tall that the filter's grid of 64 x 4 tiles would exceed 2^32 threads, iterations > 10, a sigma that is NaN or below 1e-6 (so
 * that every k_i stays finite: the centre tap's 0 * k must stay 0).
 * A denoiser owns, for one W x H on one device, the ping-pong scratch and rt_denoise's device staging (116 bytes per pixel in all), all
 * allocated by rt_denoiser_create: no call allocates on the device. rt_denoise synchronises; rt_denoise_device enqueues on `stream` (NULL = the null stream) and returns.
 * Calls on one denoiser are serialised by the denoiser: each records an event that the next call's stream waits for. */
typedef struct rt_denoise_params {
    uint32_t iterations;   /* 0 .. 10; 0 = copy                                                      */
    float sigma_color;     /* >= 1e-6, +inf = guide ignored; NaN / < 1e-6 -> RT_ERR_INVALID          */
    float sigma_normal;
    float sigma_position;  /* world units                                                            */
    float sigma_albedo;
} rt_denoise_params;       /* 20 bytes */
typedef struct rt_denoiser rt_denoiser;
int rt_denoiser_create(int device, int32_t width, int32_t height, rt_denoiser** out);
void rt_denoiser_destroy(rt_denoiser* d);
int rt_denoise(rt_denoiser* d, const rt_denoise_params* p, const float* rgba_f32, const float* albedo, const float* normal,
               const float* position, float* out_f32, uint8_t* out_u8);
int rt_denoise_device(rt_denoiser* d, const rt_denoise_params* p, const void* d_rgba_f32, const void* d_albedo, const void* d_normal,
                      const void* d_position, void* d_out_f32, void* d_out_u8, void* stream);

/* ---- Variance-guided denoising (after SVGF: Schied, Kaplanyan, Wyman, Patney, Chaitanya, Burgess, Liu, Dachsbacher, Lefohn, Salvi, HPG 2017;
 * no reference counterpart). rt_denoise's colour term has one global sigma_color; here the tolerance of every pixel is its own noise level: the
 * standard deviation of its luminance, estimated by rt_denoise_variance and carried through the filter by rt_denoise_guided. The chain is
 * rt_temporal_accumulate_moments (below) -> rt_denoise_variance -> rt_denoise_guided, or the last two alone for a still image.
 * Out of scope: feeding the first filtered iteration back into the history, and albedo demodulation.
 *
 * rt_denoiser_create_ex == rt_denoiser_create plus flags (rt_denoiser_create passes 0: the same allocation). RT_DENOISER_VARIANCE adds the host
 * variants' staging of the two calls below (an input and an output variance plane, the moments and the history lengths: 20 bytes per pixel,
 * 136 in all); the variance between iterations needs no plane, it rides in .w of the colour scratch. An unknown flag: RT_ERR_INVALID.
 *
 * Common to both calls: planes as rt_denoise's (H x W x 4 fp32 frame and guides, row 0 first); a hit is P.w finite; every operation one R1
 * fp32 op, left to right as bracketed; dot = (x*x + y*y) + z*z; exp_m and k = coefficient(sigma) = RN(1/RN(sigma*sigma)), 0 for +inf, are
 * rt_denoise's; lum(L) = (L_r*0.2126f + L_g*0.7152f) + L_b*0.0722f; L_q = (F_r*F_r, F_g*F_g, F_b*F_b) of the frame at q, as rt_denoise's step 1.
 *
 * rt_denoise_variance: out_variance (H*W floats) = the variance of every pixel's luminance. moments (H*W*2 floats, rt_temporal_accumulate_moments')
 * and history_len (H*W floats) may both be NULL (a still image; one without the other is RT_ERR_INVALID). The frame is the one the moments belong
 * to: the accumulated frame where there is temporal accumulation.
 *   Where moments are given and history_len >= (float)min_history: (m1, m2) = moments at p.
 *   Elsewhere, over the 7 x 7 window q = (x + dx, y + dy), dy = -3..3 (outer), dx = -3..3 (inner): taps outside the image are skipped, and so is
 *   a tap that differs from p in being a hit;
 *     E = (dot(N_p-N_q)*kn + dot(P_p.xyz-P_q.xyz)*kx) + dot(A_p-A_q)*ka   (a term whose coefficient is 0 is left out, E starts at +0; kn is not
 *     scaled: there is no step); w = exp_m(-E); l_q = lum(L_q); s1 += w*l_q, s2 += w*(l_q*l_q), ws += w, in tap order;
 *     m1 = s1 / ws, m2 = s2 / ws   (ws >= 1: the centre tap).
 *   var = fmax(m2 - m1*m1, 0), fmax as IEEE 754's maxNum: fmax(NaN, 0) = 0.
 *
 * rt_denoise_guided: rt_denoise with its colour term replaced; variance is H*W floats (rt_denoise_variance's), out_variance (H*W floats, may be
 * NULL) the variance of the filtered luminance. It is rt_denoise's steps 1 .. 4 with, in step 2, per iteration i (var = the input variance for
 * i = 0, then var' of the iteration before):
 *   a. g_p = sum over dy = -1..1 (outer), dx = -1..1 (inner) of (k3[dy+1]*k3[dx+1]) * var_q, k3 = {1/4, 1/2, 1/4}, q = (x + dx, y + dy) clamped
 *      into the image (not scaled by the step), g starting at +0; kl_p = 1 / (sigma_luminance * sqrt(g_p) + 1e-8f).
 *   b. E = ((fabs(l_p - l_q)*kl_p + dot(N_p-N_q)*kn_i) + dot(P_p.xyz-P_q.xyz)*kx) + dot(A_p-A_q)*ka, l = lum of this iteration's L. For
 *      sigma_luminance = +inf the term and step a are left out: the images are then rt_denoise's with sigma_color = +inf, bit for bit.
 *   c. beside S += w*L_q and Wsum += w: V += (w*w)*var_q, in tap order. L' = S / Wsum, var' = V / (Wsum*Wsum).
 *   iterations = 0: rt_denoise's step 4, and out_variance = variance.
 * Non-finite radiance (a frame may hold one: F = 1e20 gives L = +inf). There l = +inf and l*l = +inf, so moments or a window holding it have
 * m2 - m1*m1 = inf - inf = NaN and var = fmax(NaN, 0) = 0: rt_denoise_variance never returns NaN for a frame without NaN, and returns +inf only
 * where m2 overflows while m1*m1 does not. In the filter a variance of +inf gives sqrt(g) = +inf and kl = 0; a tap between a finite and an infinite
 * luminance has fabs(..) * kl = inf * 0 or E = +inf or NaN, exp_m of which is 0: its weight is 0, and 0 * inf = NaN enters S. So (sigma_luminance
 * finite) L' is NaN at every pixel with a non-finite L_q among its 25 taps, as in rt_denoise, and the region grows by 2 * step pixels per
 * iteration. The pixel that holds the non-finite value has inf - inf = NaN at its own centre tap too: all its weights are 0, Wsum = 0, and
 * there, and only there, var' = 0 / 0 = NaN as well (elsewhere V sums w*w*var_q with w = 0 and a finite var_q: it stays finite). The filter
 * does not clamp: remove fireflies before it, or accept the hole.
 * Refusals: rt_denoise's (for rt_denoise_variance out_variance is the required output), plus RT_ERR_INVALID for a denoiser created without
 * RT_DENOISER_VARIANCE. out_f32 may alias rgba_f32; no other aliasing is allowed (out_variance must not be variance). Both calls are serialised
 * with every other call on the denoiser; the host variants synchronise, the _device variants enqueue on `stream`. */
#define RT_DENOISER_VARIANCE 1u
typedef struct rt_denoise_var_params {
    uint32_t iterations;    /* 0 .. 10; 0 = copy (rt_denoise_variance ignores it, but checks it)       */
    float sigma_luminance;  /* in standard deviations; >= 1e-6, +inf = term off; NaN / < 1e-6 -> RT_ERR_INVALID */
    float sigma_normal;
    float sigma_position;   /* world units                                                             */
    float sigma_albedo;
    uint32_t min_history;   /* rt_denoise_variance: the moments are used where history_len >= this      */
} rt_denoise_var_params;    /* 24 bytes */
int rt_denoiser_create_ex(int device, int32_t width, int32_t height, uint32_t flags, rt_denoiser** out);
int rt_denoise_variance(rt_denoiser* d, const rt_denoise_var_params* p, const float* rgba_f32, const float* albedo, const float* normal,
                        const float* position, const float* moments, const float* history_len, float* out_variance);
int rt_denoise_variance_device(rt_denoiser* d, const rt_denoise_var_params* p, const void* d_rgba_f32, const void* d_albedo, const void* d_normal,
                               const void* d_position, const void* d_moments, const void* d_history_len, void* d_out_variance, void* stream);
int rt_denoise_guided(rt_denoiser* d, const rt_denoise_var_params* p, const float* rgba_f32, const float* albedo, const float* normal,
                      const float* position, const float* variance, float* out_f32, uint8_t* out_u8, float* out_variance);
int rt_denoise_guided_device(rt_denoiser* d, const rt_denoise_var_params* p, const void* d_rgba_f32, const void* d_albedo, const void* d_normal,
                             const void* d_position, const void* d_variance, void* d_out_f32, void* d_out_u8, void* d_out_variance, void* stream);

/* ---- Temporal accumulation by reprojection (no reference counterpart). Frames of an animation rendered with different seed salts
 * (rt_renderer_set_frame_seed) are independent estimates; the accumulator carries a running mean of them from frame to frame, fetched for every
 * pixel where its surface point was one frame ago (rt_scene_gbuffer_motion's prev_position, projected through the previous call's camera),
 * tested against the G-buffer and blended with the new frame. Its output is a frame in the form rt_denoise takes: temporal first, a-trous second.
 *
 * An accumulator owns, for one W x H on one device, two sets (ping-pong: taps read neighbours) of three float4 planes — history colour (linear
 * rgb, .w = the history length n, a float holding an integer), and the position and normal planes of the frame that history belongs to — and that
 * frame's camera: 96 bytes per pixel, plus the host variant's staging (88 bytes per pixel), all allocated by rt_temporal_create: no call allocates.
 * Per call, per pixel p = (x, y), with F, N, P, Q = rgba_f32, normal, position, prev_position at p and c', p00', du', dv' the camera of the
 * previous call; every operation one R1 fp32 op, left to right as bracketed; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z,
 * cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), each product and difference one op:
 *   1. L = (F_r*F_r, F_g*F_g, F_b*F_b): linear radiance, as rt_denoise's step 1.
 *   2. p has NO HISTORY when there is no previous call since create / reset, when p is a miss (P.w not finite), or when step 3, 4 or 5 fails.
 *      Then L' = L, n' = 1 for a hit and 0 for a miss, and the outputs at p are the input's own: out_f32 = (F_r, F_g, F_b, 1) and its to_unorm8
 *      (not a square root of a square).
 *   3. r = Q.xyz - c'; m = cross(du', dv'); e = p00' - c'; s = dot(e, m) / dot(r, m); fail unless s is finite and > 0. h = r*s - e;
 *      sx = dot(h, du') / dot(du', du'), sy = dot(h, dv') / dot(dv', dv'); fail unless -1 < sx < (float)W and -1 < sy < (float)H (NaN fails, before
 *      any conversion to an integer). The centre of pixel column x is sx = x. (du' and dv' are taken to be perpendicular, as rt_camera_init makes
 *      them: for a sheared pixel grid sx, sy are not the grid's coordinates.)
 *   4. x0 = floor(sx), fx = sx - x0, likewise y0, fy. Four taps t = (x0 + i, y0 + j) in the order (i, j) = (0,0), (1,0), (0,1), (1,1), with the
 *      weight w_t = (i ? fx : 1 - fx) * (j ? fy : 1 - fy). A tap is VALID when it lies in the image, w_t > 0, its stored n_t >= 1 (it was a hit),
 *      dot(d, d) * kx <= 1 for d = Ppos_t.xyz - Q.xyz (kx = RN(1 / RN(sigma_position^2)), rt_denoise's coefficient; for sigma = +inf kx = 0 and
 *      the test is left out) and dot(N.xyz, Pnrm_t.xyz) >= cos_normal (cos_normal = -1: the test is left out). Wsum and S accumulate w_t and
 *      w_t * Lhist_t over the valid taps in tap order; fail when Wsum < 1/64. Hc = S / Wsum; n_prev = the MINIMUM n_t of the valid taps (it stays
 *      an exact integer and is conservative at disocclusion edges).
 *   5. n' = min(n_prev + 1, max_history). n' == 1 (only with max_history = 1): no history (step 2). Otherwise a = 1 / n';
 *      L' = Hc + (L - Hc) * a per channel.
 *   6. The current set becomes colour (L', n'), position P, normal N, camera cam. Where p had history: out_f32 = (sqrt(L'), 1), out_u8 = its
 *      to_unorm8 with alpha 255; everywhere history_len = n'.
 * Limits: reflections and refractions are reprojected with the surface they appear on (history on mirrors and glass lags the motion of what they
 * show); lighting that changes on a static surface lags by up to max_history frames.
 * Refused with RT_ERR_INVALID, before any HIP call: NULL handles or required pointers, out_f32 and out_u8 both NULL, device < 0, non-positive
 * sizes, W * H >= 2^31, a shape so narrow and tall that the grid of 64 x 4 tiles would exceed 2^32 threads, max_history outside 1 .. 4096, a
 * sigma_position that is NaN or below 1e-6, cos_normal NaN or outside [-1, 1], a camera whose width or height is not the accumulator's.
 * history_len (H*W floats) may be NULL. out_f32 may alias rgba_f32 (in place); no other aliasing is allowed.
 * rt_temporal_accumulate takes host arrays and synchronises; rt_temporal_accumulate_device takes device arrays and enqueues one kernel on
 * `stream` (NULL = the null stream). Calls on one accumulator are serialised by the accumulator: each records an event that the next call's
 * stream waits for. rt_temporal_reset forgets the history: the next call passes its frame through. */
typedef struct rt_temporal_params {
    uint32_t max_history;  /* 1 .. 4096: the blend weight never drops below 1 / max_history; 1 = pass-through */
    float sigma_position;  /* world units, >= 1e-6 or +inf (test off)                                         */
    float cos_normal;      /* -1 .. 1; -1 = test off                                                           */
} rt_temporal_params;      /* 12 bytes */
typedef struct rt_temporal rt_temporal;
int rt_temporal_create(int device, int32_t width, int32_t height, rt_temporal** out);
void rt_temporal_destroy(rt_temporal* t);
int rt_temporal_reset(rt_temporal* t);
int rt_temporal_accumulate(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const float* rgba_f32, const float* normal,
                           const float* position, const float* prev_position, float* out_f32, uint8_t* out_u8, float* history_len);
int rt_temporal_accumulate_device(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const void* d_rgba_f32, const void* d_normal,
                                  const void* d_position, const void* d_prev_position, void* d_out_f32, void* d_out_u8, void* d_history_len,
                                  void* stream);

/* Temporal luminance moments, for rt_denoise_variance. rt_temporal_create_ex == rt_temporal_create plus flags (rt_temporal_create passes 0: the
 * same allocation). With RT_TEMPORAL_MOMENTS the accumulator also owns two (ping-pong) planes of float2 moments, 8 bytes per pixel each, and the
 * host variant's staging of them (8 more). An unknown flag: RT_ERR_INVALID.
 * rt_temporal_accumulate_moments[_device] is rt_temporal_accumulate[_device] with one more output, moments (H*W*2 floats, required): its colour
 * outputs and history_len are rt_temporal_accumulate's bit for bit. Added to that contract's steps, with lum(L) = (L_r*0.2126f + L_g*0.7152f) +
 * L_b*0.0722f of step 1's L:
 *   l = lum(L), M = (l, l*l). No history (step 2): M' = M. With history: Sm accumulates w_t * Mhist_t per component over step 4's valid taps, in
 *   their order and with their weights; Hm = Sm / Wsum; M' = Hm + (M - Hm) * a per component, a of step 5. The current set keeps M'; moments = M'.
 * M' is the running mean of l and of l*l over the frames the colour is the mean of. A non-finite L makes them +inf or NaN: see rt_denoise_variance.
 * RT_ERR_INVALID on an accumulator created without the flag. A plain rt_temporal_accumulate[_device] on an accumulator WITH the flag is allowed
 * and keeps the moments consistent: it computes and stores M' as above (the same kernel) and only does not return it. */
#define RT_TEMPORAL_MOMENTS 1u
int rt_temporal_create_ex(int device, int32_t width, int32_t height, uint32_t flags, rt_temporal** out);
int rt_temporal_accumulate_moments(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const float* rgba_f32, const float* normal,
                                   const float* position, const float* prev_position, float* out_f32, uint8_t* out_u8, float* history_len,
                                   float* moments);
int rt_temporal_accumulate_moments_device(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam, const void* d_rgba_f32,
                                          const void* d_normal, const void* d_position, const void* d_prev_position, void* d_out_f32, void* d_out_u8,
                                          void* d_history_len, void* d_moments, void* stream);

/* ---- Multi-GPU frame gather over xGMI (no reference counterpart: the reference renders on ONE device and hands its
 * single image to stbi_write_png, src/main.cpp:57-70, src/util.hpp:8-33). SURVEY §8(e): the frame is split into interleaved
 * strips (rt_renderer_set_tile), every GPU renders its strips into its own compact device buffer, and ONE collective brings
 * them to the root GPU: ncclGather of the per-GPU strip buffers (rccl.h: ncclCommInitAll / ncclGroupStart / ncclGather /
 * ncclGroupEnd) followed by a de-interleave kernel on the root. The frame touches host memory only when the caller asks
 * for it (the PNG). librccl.so is loaded on first use (dlopen): single-GPU callers never load it.
 *
 * One process drives all devices (the C++ adapter's `--devices A,B,..`); the one-process-per-GPU form of the same gather is
 * torch.distributed (backend nccl = RCCL) in rtamd/dist.py. */
typedef struct rt_comm rt_comm;
/* Communicator over `n` devices, rank i on devices[i]; rank 0 is the root. If the same device appears more than once
 * (rehearsal of an n-GPU split on fewer GPUs) RCCL cannot be used (one rank per device): the gather then moves the strips
 * with device-to-device copies and runs the same de-interleave kernel; rt_comm_uses_rccl() tells which. */
int rt_comm_create(int n, const int* devices, rt_comm** out);
void rt_comm_destroy(rt_comm* c);
int rt_comm_uses_rccl(const rt_comm* c);
/* The renderer's own device buffers of its tile (local_rows x W x 4 floats / bytes): render into them without any host copy
 * with rt_render_frame_begin(r, cam, rt_renderer_tile_f32(r), rt_renderer_tile_u8(r), NULL) + rt_render_frame_end. */
void* rt_renderer_tile_f32(rt_renderer* r);
void* rt_renderer_tile_u8(rt_renderer* r);
/* Gathers the last frame of renderers[0..n-1] — renderer i must be tile (i, n, strip_rows) of one W x H frame on devices[i],
 * rendered into its own tile buffers — into the full frame on the root device and, if the pointers are not NULL, copies it
 * to the host (rgba_f32: H*W*4 floats, rgba_u8: H*W*4 bytes; the f32 / u8 planes are only gathered when asked for here or
 * through want_device_*). The device-resident frame stays valid until the next gather: rt_comm_frame_f32 / _u8. */
int rt_frame_gather(rt_comm* c, rt_renderer* const* renderers, float* rgba_f32, uint8_t* rgba_u8, int want_device_f32,
                    int want_device_u8);
/* The same in two calls. _begin only ENQUEUES the collective and the de-interleave (event waits between the renderers' streams
 * and the root's; no host wait): a renderer's next frame may be begun right after it and overlaps with the gather. rt_comm_wait
 * blocks until the gathered frame is complete on the root device and copies it to the host where a pointer is given.
 * If a collective fails half-way the communicator is marked unusable (every later call returns RT_ERR_HIP): destroy it and
 * create a new one. */
int rt_frame_gather_begin(rt_comm* c, rt_renderer* const* renderers, int want_f32, int want_u8);
int rt_comm_wait(rt_comm* c, float* rgba_f32, uint8_t* rgba_u8);
int rt_comm_size(const rt_comm* c); /* ranks of the communicator (with RCCL: what ncclCommInitAll was given) */
const void* rt_comm_frame_f32(const rt_comm* c);
const void* rt_comm_frame_u8(const rt_comm* c);

/* ---- Device unit probes (parity tests of the building blocks; tiny launches) --------------- */
/* XorShift32State::operator() (src/xorshift.hpp:11-20) run on the device: n draws from `seed`. */
int rt_probe_xorshift(int device, uint32_t seed, uint32_t n, float* out, uint32_t* state_out);
/* float -> half -> float round trip as RayData stores dir/att/rad (src/camera.hpp:18-43). */
int rt_probe_half_roundtrip(int device, uint32_t n, const float* in, float* out,
                            uint16_t* bits_out);
/* Material::scatter (src/material.hpp:211-224) on the device for n independent inputs:
 * dir/normal: 3n, uv: 2n, seed: n. Outputs ok (n, 0/1), out_dir 3n, out_att 3n, seed_out n. */
int rt_probe_scatter(rt_scene* scene, uint32_t material, uint32_t n, const float* dir,
                     const float* normal, const float* uv, const uint32_t* seed, uint8_t* ok,
                     float* out_dir, float* out_att, uint32_t* seed_out);

/* The kernels' short forms of RN(1 / x) and RN(1 / RN(sqrt(x))) (rt_device.h: rcp_rn, inv_sqrt2; glm::normalize as src/trace_ray.hpp and
 * src/material.hpp use it, the 1 / det of the triangle test) against the IEEE expressions, on ALL 2^32 float bit patterns:
 * mismatches[0], mismatches[1] = inputs on which they differ. The arithmetic contract requires both to be 0. ~1 s. */
int rt_probe_rounding(int device, uint64_t* mismatches);

/* The origin skip's per-ray test on n rays: ray i (org, dir: 3n floats) is tested against entry i of `entries` (8 words each, the
 * layout of a scene's skip table: child word, normal, first vertex, two half thresholds). word_device receives the word the render kernels would
 * keep for the ray — the entry's child word, or the no-match word 1 — computed by a kernel that reads the entry as they do; word_host the
 * same function compiled for the host, as the host walk (rt_scene_count_visits mode 4) applies it. Either output may be NULL. device < 0: the host
 * form alone, no device call (word_device must be NULL). The two must agree on every input, NaN, infinities and subnormals included. */
int rt_probe_origin_skip(int device, uint32_t n, const uint32_t* entries, const float* org, const float* dir,
                         uint32_t* word_device, uint32_t* word_host);

const char* rt_last_error(void);
int rt_abi_version(void);
/* Number of HIP devices visible, or a negative rt_status. */
int rt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
