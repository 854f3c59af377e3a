// scene_rules_check: the scene's geometry rules (csrc/scene_rules.h) against the host builder and the host refit, on a small random tree: a few
// dozen triangles over two instances with distinct transforms. Host only; built with the host's AddressSanitizer and UBSan by
// tests/test_host_cpp.py, which links it with scene_build.cpp and scene_check.cpp. On the same tree it runs the four host walks of
// scene_check.cpp (closest_host, nearest_host, multihit_host, count_visits), so their shared steps and list run under the sanitizers: every
// walk of the tree against its own brute force. Prints "ok <checks>" and returns 0, or says what differs.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "scene_build.h"
#include "scene_rules.h"

using namespace rt;

namespace rt { // (the device builder is no part of this program: the host builders never call it)
int build_lbvh_gpu(HostScene&, const std::vector<TriRec>&, std::string& err) { return err = "no device", RT_ERR_NO_DEVICE; }
} // namespace rt

static long g_checks = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        ++g_checks;                                   \
        if (!(cond)) {                                \
            std::printf("FAILED %s: ", #cond);        \
            std::printf(__VA_ARGS__);                 \
            std::printf("\n");                        \
            return 1;                                 \
        }                                             \
    } while (0)

static bool same(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

struct Desc {
    std::vector<float> pos, nrm, uv;
    std::vector<uint32_t> idx, tri_inst;
    std::vector<rt_instance> inst;
    rt_material mat{};
    rt_scene_desc d{};
    const rt_scene_desc* get() {
        d.n_vertices = (uint32_t)(pos.size() / 3), d.positions = pos.data(), d.normals = nrm.data(), d.uvs = uv.data();
        d.n_triangles = (uint32_t)tri_inst.size(), d.indices = idx.data(), d.tri_instance = tri_inst.data();
        d.n_instances = (uint32_t)inst.size(), d.instances = inst.data();
        d.n_materials = 1, d.materials = &mat;
        d.n_layers = 0, d.textures = nullptr;
        d.sky[0] = 0.5f, d.sky[1] = 0.7f, d.sky[2] = 1.0f;
        return &d;
    }
};

// a rotation about (1, 2, 3) with a non-uniform scale and a translation; the normal matrix is data to the builder
static rt_instance instance(float angle, float sx, float sy, float sz, float tx, float ty, float tz) {
    rt_instance in{};
    const double n = std::sqrt(14.0), ax[3] = {1 / n, 2 / n, 3 / n}, c = std::cos(angle), s = std::sin(angle);
    const float sc[3] = {sx, sy, sz};
    for (int col = 0; col < 3; ++col)
        for (int row = 0; row < 3; ++row) {
            const double cross = row == col ? 0.0 : ((row - col + 3) % 3 == 1 ? ax[3 - row - col] : -ax[3 - row - col]);
            const double r = (row == col ? c : 0.0) + (1 - c) * ax[row] * ax[col] + s * cross;
            in.transform[4 * col + row] = (float)r * sc[col];
            in.normal_mat[3 * col + row] = (float)r / sc[col];
        }
    in.transform[12] = tx, in.transform[13] = ty, in.transform[14] = tz, in.transform[15] = 1.0f;
    in.material = 0;
    return in;
}

static Desc random_scene(uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    Desc s;
    const uint32_t tris_of[2] = {29, 18};
    for (uint32_t i = 0; i < 2; ++i)
        for (uint32_t t = 0; t < tris_of[i]; ++t) {
            const float c[3] = {4.0f * u(rng), 4.0f * u(rng), 4.0f * u(rng)};
            for (int k = 0; k < 3; ++k) {
                s.idx.push_back((uint32_t)(s.pos.size() / 3));
                for (int a = 0; a < 3; ++a) s.pos.push_back(c[a] + 0.4f * u(rng)), s.nrm.push_back(u(rng));
                s.uv.push_back(u(rng)), s.uv.push_back(u(rng));
            }
            s.tri_inst.push_back(i);
        }
    s.inst = {instance(0.7f, 1.5f, 0.8f, 1.1f, 3.0f, -1.0f, 0.5f), instance(-2.1f, 0.6f, 1.3f, 0.9f, -6.0f, 2.0f, 4.0f)};
    s.mat.type = 0, s.mat.color[0] = s.mat.color[1] = s.mat.color[2] = 0.5f, s.mat.ior = 1.5f;
    return s;
}

// the nodes' exact boxes by the shared refit, node by node in level order; false where the quantiser refuses
static bool refit_by_rule(HostScene& hs, const std::vector<uint32_t>& level_nodes, std::vector<Box3>& box) {
    box.assign(hs.nodes.size(), empty_box());
    for (uint32_t i : level_nodes) {
        BvhNode q;
        const RefitResult res = refit_node(
            hs.nodes[i], [&](int32_t child) { return box[(size_t)child]; }, [&](uint32_t r) { return &hs.wverts[9 * (size_t)hs.tris[r].global_index]; },
            hs.pad, box[i], q);
        if (res == kRefitRefused) return false;
        if (res == kRefitDone) hs.nodes[i] = q;
    }
    return true;
}

static bool inside(const Box3& inner, const Box3& outer) {
    for (int a = 0; a < 3; ++a)
        if (!(outer.lo[a] <= inner.lo[a] && inner.hi[a] <= outer.hi[a])) return false;
    return true;
}

// The host walks on the built tree: 48 points around the scene and 48 rays through triangle centroids. The walk of every query equals its
// brute force bit for bit (this scene has no sliver: the multi-hit contract's limit does not bite), a list of one is the closest point or
// the closest hit, a page behind the first entry's key is the list shifted by one, and every box mode of count_visits finds the same hits.
static int check_walks(const HostScene& hs, int kind) {
    constexpr uint32_t n = 48, kmax = 8;
    std::mt19937 rng(1234u + (uint32_t)kind);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    const size_t T = hs.wverts.size() / 9;
    std::vector<float> pos(3 * n), org(3 * n), dir(3 * n), md2(n), tmax(n);
    for (uint32_t i = 0; i < n; ++i) {
        const float* w = &hs.wverts[9 * (size_t)(rng() % T)];
        for (int a = 0; a < 3; ++a) {
            pos[3 * i + a] = 12.0f * u(rng);
            org[3 * i + a] = 40.0f * u(rng);
            dir[3 * i + a] = ((w[a] + w[3 + a] + w[6 + a]) / 3.0f - org[3 * i + a]) * (1.0f + 0.5f * u(rng));
        }
    }
    std::string err;
    uint64_t nv = 0, nt = 0;
    struct Slots {
        std::vector<float> t, u, v;
        std::vector<uint32_t> tri, count;
        explicit Slots(size_t k) : t(n * k), u(n * k), v(n * k), tri(n * k), count(n) {}
        bool operator==(const Slots& o) const {
            return same(t.data(), o.t.data(), 4 * t.size()) && same(u.data(), o.u.data(), 4 * u.size()) && same(v.data(), o.v.data(), 4 * v.size()) && tri == o.tri && count == o.count;
        }
    };
    // closest_host: brute force and walk
    std::vector<float> cd[2] = {std::vector<float>(n), std::vector<float>(n)}, cpt[2] = {std::vector<float>(3 * n), std::vector<float>(3 * n)};
    std::vector<uint32_t> ctri[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
    for (int bvh = 0; bvh < 2; ++bvh)
        CHECK(closest_host(hs, n, pos.data(), nullptr, bvh, cd[bvh].data(), nullptr, nullptr, ctri[bvh].data(), cpt[bvh].data(), &nv, &nt, err) == RT_OK, "closest_host: %s", err.c_str());
    CHECK(ctri[0] == ctri[1] && same(cd[0].data(), cd[1].data(), 4 * n) && same(cpt[0].data(), cpt[1].data(), 12 * n), "closest_host: the walk differs from the brute force");
    CHECK(nv > 0 && nt > 0 && nt < (uint64_t)n * hs.tris.size(), "closest_host: the walk culled nothing");
    for (int ray = 0; ray < 2; ++ray) {
        const char* what = ray ? "multihit_host" : "nearest_host";
        auto run = [&](uint32_t k, const float* lim, const float* kt, const uint32_t* ktri, int bvh, Slots& s) {
            return ray ? multihit_host(hs, n, k, org.data(), dir.data(), lim, kt, ktri, bvh, s.t.data(), s.u.data(), s.v.data(), s.tri.data(), s.count.data(), &nv, &nt, err)
                       : nearest_host(hs, n, k, pos.data(), lim, kt, ktri, bvh, s.t.data(), s.u.data(), s.v.data(), s.tri.data(), s.count.data(), &nv, &nt, err);
        };
        Slots all(kmax);
        CHECK(run(kmax, nullptr, nullptr, nullptr, 0, all) == RT_OK, "%s: %s", what, err.c_str());
        std::vector<float> lim(n), kt(n);
        std::vector<uint32_t> ktri(n);
        for (uint32_t i = 0; i < n; ++i) { // the limit ON the third entry, the key on the first (a miss: +inf and kNoTri, nothing behind it)
            lim[i] = all.t[kmax * i + 2], kt[i] = all.t[kmax * i], ktri[i] = all.tri[kmax * i];
            for (uint32_t s = 1; s < kmax; ++s)
                CHECK(all.tri[kmax * i + s] == kNoTri || all.t[kmax * i + s - 1] < all.t[kmax * i + s] ||
                          (all.t[kmax * i + s - 1] == all.t[kmax * i + s] && all.tri[kmax * i + s - 1] < all.tri[kmax * i + s]), "%s: entry %u is not sorted", what, i);
        }
        for (uint32_t k : {1u, 3u, kmax})
            for (int keyed = 0; keyed < 2; ++keyed)
                for (int limited = 0; limited < 2; ++limited) {
                    Slots brute(k), walk(k);
                    for (int bvh = 0; bvh < 2; ++bvh)
                        CHECK(run(k, limited ? lim.data() : nullptr, keyed ? kt.data() : nullptr, keyed ? ktri.data() : nullptr, bvh, bvh ? walk : brute) == RT_OK, "%s: %s", what, err.c_str());
                    CHECK(brute == walk, "%s k = %u key %d limit %d: the walk differs from the brute force", what, k, keyed, limited);
                    for (uint32_t i = 0; i < n; ++i) {
                        uint32_t first = 0, avail = 0; // of the list of kmax: the entries not behind the key, and those that count
                        for (uint32_t s = 0; s < all.count[i]; ++s) {
                            const float t = all.t[kmax * i + s];
                            if (keyed && !(t > kt[i] || (t == kt[i] && all.tri[kmax * i + s] > ktri[i]))) first++;
                            else if (!limited || t <= lim[i]) avail++;
                        }
                        const bool goes_on = all.count[i] == kmax && (!limited || all.t[kmax * i + kmax - 1] <= lim[i]); // more may count behind it
                        const uint32_t want = std::min(avail, k);
                        CHECK(goes_on && avail < k ? brute.count[i] >= avail : brute.count[i] == want, "%s k = %u key %d limit %d: entry %u counts %u, the list of %u says %u",
                              what, k, keyed, limited, i, brute.count[i], kmax, want);
                        for (uint32_t s = 0; s < want; ++s)
                            CHECK(brute.tri[k * i + s] == all.tri[kmax * i + first + s] && same(&brute.t[k * i + s], &all.t[kmax * i + first + s], 4), "%s: entry %u slot %u", what, i, s);
                    }
                }
        if (!ray) {
            for (uint32_t i = 0; i < n; ++i) CHECK(all.tri[kmax * i] == ctri[0][i] && same(&all.t[kmax * i], &cd[0][i], 4), "nearest_host: the first entry is not closest_host's");
        } else {
            std::vector<float> t(n);
            std::vector<uint32_t> tri(n), hits(n);
            for (int mode : {0, 1, 2}) {
                std::fill(tri.begin(), tri.end(), kNoTri);
                CHECK(count_visits(hs, n, org.data(), dir.data(), mode, &nv, &nt, t.data(), tri.data(), err) == RT_OK, "count_visits mode %d: %s", mode, err.c_str());
                for (uint32_t i = 0; i < n; ++i) CHECK(tri[i] == all.tri[kmax * i], "count_visits mode %d: ray %u hits %u, the list's first entry is %u", mode, i, tri[i], all.tri[kmax * i]);
                if (mode == 0) hits = tri;
            }
            // mode 4: the rays go on from their hits, starting on the triangle they hit; with the skip they find what they find without it
            std::vector<float> o2(org);
            for (uint32_t i = 0; i < n; ++i)
                for (int a = 0; a < 3 && hits[i] != kNoTri; ++a) o2[3 * i + a] = org[3 * i + a] + dir[3 * i + a] * all.t[kmax * i];
            std::vector<uint32_t> plain(n, kNoTri), skipped(hits);
            uint64_t nv0 = 0;
            CHECK(count_visits(hs, n, o2.data(), dir.data(), 0, &nv0, &nt, t.data(), plain.data(), err) == RT_OK, "count_visits: %s", err.c_str());
            CHECK(count_visits(hs, n, o2.data(), dir.data(), 4, &nv, &nt, t.data(), skipped.data(), err) == RT_OK, "count_visits mode 4: %s", err.c_str());
            CHECK(plain == skipped && nv <= nv0, "count_visits mode 4: the skip changed a hit or added a visit");
        }
    }
    return 0;
}

static int check_builder(int kind, Desc& sd) {
    const rt_scene_desc* d = sd.get();
    HostScene hs;
    std::string err;
    CHECK(build_host_scene(d, kind, hs, err) == RT_OK, "builder %d: %s", kind, err.c_str());
    CHECK(hs.n_split_triangles == 0 && hs.built_by == kind, "builder %d: not a tree of exact unions", kind);
    const uint32_t T = d->n_triangles;
    std::vector<uint64_t> use(d->n_instances, 0);
    for (uint32_t t = 0; t < T; ++t) use[d->tri_instance[t]]++;
    std::vector<InstRec> rows;
    std::vector<uint32_t> slot;
    shading_rows(d->instances, d->n_instances, use, hs.packed_mat, rows, slot);
    // the rules one by one against what flatten() left in the built scene
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t ii = d->tri_instance[t];
        float w[9];
        for (int k = 0; k < 3; ++k) {
            const float* p = d->positions + 3 * (size_t)d->indices[3 * t + k];
            for (int a = 0; a < 3; ++a) w[3 * k + a] = world_coord(d->instances[ii].transform, a, p[0], p[1], p[2]);
        }
        CHECK(same(w, &hs.wverts[9 * (size_t)t], 36), "world vertices of triangle %u", t);
        ShadeRec sr{};
        shade_normals(sr, d->indices + 3 * (size_t)t, d->normals);
        CHECK(same(sr.n0, hs.shade[t].n0, 36), "normals of triangle %u", t);
        CHECK(shading_word(hs.packed_mat, slot[ii], d->instances[ii].material, ii) == hs.shade[t].instance, "shading word of triangle %u", t);
    }
    if (check_walks(hs, kind)) return 1;
    const std::vector<BvhNode> built_nodes = hs.nodes;
    const std::vector<TriRec> built_tris = hs.tris;
    for (size_t r = 0; r < hs.tris.size(); ++r) {
        TriRec tr{};
        tri_record(&hs.wverts[9 * (size_t)hs.tris[r].global_index], tr.v0, tr.e1, tr.e2);
        CHECK(same(tr.v0, built_tris[r].v0, 36), "leaf record %zu", r);
    }
    record_boxes(hs);
    for (size_t r = 0; r < hs.tris.size(); ++r) {
        const Box3 b = tri_box(&hs.wverts[9 * (size_t)hs.tris[r].global_index]);
        CHECK(same(b.lo, &hs.rec_lo[3 * r], 12) && same(b.hi, &hs.rec_hi[3 * r], 12), "box of leaf record %zu", r);
    }
    // unchanged vertices: refit_host and the rule applied node by node both give the built tree back, words 0..11 and the leaf records
    std::vector<uint32_t> level_nodes, level_start;
    node_levels(hs.nodes, level_nodes, level_start);
    CHECK(level_nodes.size() == hs.nodes.size(), "builder %d: %zu of %zu nodes reached", kind, level_nodes.size(), hs.nodes.size());
    std::vector<float> box;
    HostScene refit = hs;
    CHECK(refit_host(refit, level_nodes, box, err), "refit_host: %s", err.c_str());
    HostScene ruled = hs;
    std::vector<Box3> rbox;
    CHECK(refit_by_rule(ruled, level_nodes, rbox), "refit_node refused a node of the built tree");
    for (size_t i = 0; i < hs.nodes.size(); ++i) {
        CHECK(same(&refit.nodes[i], &built_nodes[i], 64), "refit_host: node %zu of builder %d", i, kind);
        CHECK(same(&ruled.nodes[i], &built_nodes[i], 64), "refit_node: node %zu of builder %d", i, kind);
        CHECK(same(&rbox[i], &box[6 * i], 24), "exact box of node %zu", i);
    }
    for (size_t r = 0; r < hs.tris.size(); ++r) CHECK(same(&refit.tris[r], &built_tris[r], sizeof(TriRec)), "refit_host: leaf record %zu", r);
    // every vertex moved: each node's decoded child boxes contain their children's exact boxes
    std::mt19937 rng(99u + (uint32_t)kind);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<float> pos(sd.pos);
    for (float& p : pos) p += 0.75f * u(rng);
    const std::vector<rt_instance> inst = {instance(1.9f, 0.9f, 1.4f, 0.7f, -2.0f, 5.0f, 1.0f), instance(0.4f, 1.2f, 0.5f, 1.6f, 7.0f, -3.0f, -2.0f)};
    HostScene moved = hs;
    world_vertices(T, d->indices, d->tri_instance, inst.data(), pos.data(), moved.wverts);
    CHECK(world_bounds(moved.wverts, moved.bounds_lo, moved.bounds_hi, moved.pad, err), "world_bounds: %s", err.c_str());
    CHECK(!same(moved.wverts.data(), hs.wverts.data(), 4 * hs.wverts.size()), "the vertices did not move");
    CHECK(refit_host(moved, level_nodes, box, err), "refit_host after the move: %s", err.c_str());
    CHECK(check_bvh(moved, err) == RT_OK, "check_bvh after the move: %s", err.c_str());
    for (size_t i = 0; i < moved.nodes.size(); ++i)
        for (int k = 0; k < 4 && moved.nodes[i].child[k] != kChildEmpty; ++k) {
            const int32_t c = moved.nodes[i].child[k];
            CHECK(c == built_nodes[i].child[k], "child word %d of node %zu changed", k, i);
            Box3 exact = empty_box();
            if (c >= 0) std::memcpy(&exact, &box[6 * (size_t)c], 24);
            else
                for (uint32_t r = leaf_range(c).first; r < leaf_range(c).first + leaf_range(c).count; ++r)
                    grow(exact, tri_box(&moved.wverts[9 * (size_t)moved.tris[r].global_index]));
            CHECK(inside(exact, child_box(moved.nodes[i], k)), "child %d of node %zu is not inside its decoded box", k, i);
        }
    return 0;
}

int main() {
    Desc sd = random_scene(7);
    for (int kind : {RT_BVH_LBVH, RT_BVH_SAH})
        if (check_builder(kind, sd)) return 1;
    // the two forms of a child word
    for (int32_t c : {0, 1, 341, 0x7FFFFFFF / 64, leaf_child(0, 1), leaf_child(12345, 2), kChildEmpty}) {
        ++g_checks;
        if (host_child_word(device_child_word(c)) != c) return std::printf("FAILED child word %d\n", c), 1;
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
