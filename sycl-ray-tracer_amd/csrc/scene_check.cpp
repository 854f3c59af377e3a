// scene_check.cpp — host diagnostics of a built scene: the two surface-area costs rt_scene_info reports, the structural check behind
// rt_scene_check_bvh and the node-visit count behind rt_scene_count_visits. Nothing here decides anything about a tree or a render.
#include "scene_build.h"
#include "scene_rules.h"
#include "rt_closest_point.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace rt {
namespace {

// Depth-first walk below `child`: r receives the exact bounds of everything below it, visit(node, k, box) the exact subtree box of every
// child k of every inner node on the way (children before their parents). enter(child, depth) runs before a child is read; either
// callback stops the walk by returning false, and so does the walk itself.
template <class Enter, class Visit>
bool exact_boxes(const HostScene& hs, int32_t child, uint32_t depth, Box3& r, Enter&& enter, Visit&& visit) {
    r = empty_box();
    if (!enter(child, depth)) return false;
    if (child < 0) {
        r = leaf_bounds(hs, child);
        return true;
    }
    const BvhNode& n = hs.nodes[(size_t)child];
    for (int k = 0; k < 4; ++k) {
        if (n.child[k] == kChildEmpty) continue;
        Box3 c;
        if (!exact_boxes(hs, n.child[k], depth + 1, c, enter, visit) || !visit(child, k, c)) return false;
        grow(r, c);
    }
    return true;
}

} // namespace

// Surface-area cost of a device-built tree (the diagnostic rt_scene_info reports for the host builders too): every node's children boxes
// decoded, inner child 1 step x area, leaf child (triangles) x area, relative to the root's area.
double decoded_sah_cost(const HostScene& hs) {
    double cost = 0.0, root_area = 0.0;
    for (size_t i = 0; i < hs.nodes.size(); ++i) {
        const BvhNode& n = hs.nodes[i];
        Box3 nb = empty_box();
        for (int k = 0; k < 4; ++k) {
            if (n.child[k] == kChildEmpty) continue;
            const Box3 b = child_box(n, k);
            grow(nb, b);
            const double w = n.child[k] >= 0 ? 1.0 : (double)leaf_range(n.child[k]).count;
            cost += w * (double)half_area(b.lo, b.hi);
        }
        if (i == 0) root_area = (double)half_area(nb.lo, nb.hi);
    }
    return root_area > 0.0 ? 1.0 + cost / root_area : 0.0;
}

double refit_sah_cost(const HostScene& hs, const std::vector<float>& box) {
    if (hs.built_by == RT_BVH_LBVH_GPU) return decoded_sah_cost(hs); // the measure its build reported: the same tree, the same cost
    if (hs.nodes.empty() || box.size() < 6 * hs.nodes.size()) return 0.0;
    const double root_area = std::max(1e-30, (double)half_area(&box[0], &box[3]));
    double cost = 0.0;
    for (const BvhNode& n : hs.nodes)
        for (int k = 0; k < 4; ++k) {
            if (n.child[k] == kChildEmpty) continue;
            if (n.child[k] >= 0) {
                cost += (double)half_area(&box[6 * (size_t)n.child[k]], &box[6 * (size_t)n.child[k] + 3]) / root_area;
            } else {
                const Box3 b = leaf_bounds(hs, n.child[k]);
                cost += (double)half_area(b.lo, b.hi) / root_area * (double)leaf_range(n.child[k]).count;
            }
        }
    return 1.0 + cost;
}

// ---- the origin skip: the proof behind one table entry (rt_types.h: SkipRec) ------------------------------------------------------
uint16_t half_up(double x) {
    if (!(x >= 0.0)) return 0x7C00;
    if (x > 65504.0) return 0x7C00;
    const _Float16 h = (_Float16)x; // round to nearest even
    uint16_t b;
    std::memcpy(&b, &h, 2);
    if ((double)h < x) b++; // positive and finite: the next half up (65504 was the largest x)
    return b;
}
float half_value(uint16_t bits) {
    _Float16 h;
    std::memcpy(&h, &bits, 2);
    return (float)h;
}

namespace {
// the leaf records below `child`, at most kSkipMaxRecords of them (false: more)
bool records_below(const HostScene& hs, int32_t child, uint32_t depth, std::vector<uint32_t>& out) {
    if (child == kChildEmpty) return true;
    if (child < 0) {
        const LeafRange leaf = leaf_range(child);
        if ((size_t)leaf.first + leaf.count > hs.tris.size()) return false;
        for (uint32_t k = 0; k < leaf.count; ++k) out.push_back(leaf.first + k);
        return out.size() <= kSkipMaxRecords;
    }
    if ((size_t)child >= hs.nodes.size() || depth >= (uint32_t)kStackSize) return false;
    for (int k = 0; k < 4; ++k)
        if (!records_below(hs, hs.nodes[(size_t)child].child[k], depth + 1, out)) return false;
    return true;
}
} // namespace

bool skip_bounds(const HostScene& hs, const float nf[3], const float pf[3], int32_t child, double& a0, double& a2) {
    std::vector<uint32_t> recs;
    if (!records_below(hs, child, 0, recs) || recs.empty()) return false;
    const double n[3] = {nf[0], nf[1], nf[2]}, p[3] = {pf[0], pf[1], pf[2]};
    const double nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(std::fabs(nn - 1.0) <= 1e-6)) return false;
    double dev = 0.0, reach = 0.0, kappa = 1.0;
    for (uint32_t r : recs) {
        const TriRec& tr = hs.tris[r];
        const double e1[3] = {tr.e1[0], tr.e1[1], tr.e1[2]}, e2[3] = {tr.e2[0], tr.e2[1], tr.e2[2]};
        const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double area2 = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
        if (!(area2 >= 1e-24) || !std::isfinite(area2)) return false;
        kappa = std::max(kappa, l1 * l2 / area2);
        double plus = 0.0, minus = 0.0; // |n' - n|^2, |n' + n|^2
        for (int a = 0; a < 3; ++a) plus += (c[a] / area2 - n[a]) * (c[a] / area2 - n[a]), minus += (c[a] / area2 + n[a]) * (c[a] / area2 + n[a]);
        if (!(std::sqrt(std::min(plus, minus)) <= 0.9 / 1024.0)) return false;
        for (int v = 0; v < 3; ++v) { // the triangle the kernels test: v0, v0 + e1, v0 + e2
            double s = 0.0, d2 = 0.0;
            for (int a = 0; a < 3; ++a) {
                const double x = (double)tr.v0[a] + (v == 1 ? e1[a] : (v == 2 ? e2[a] : 0.0)) - p[a];
                s += n[a] * x, d2 += x * x;
            }
            dev = std::max(dev, std::fabs(s)), reach = std::max(reach, std::sqrt(d2));
        }
    }
    if (!(kappa <= 256.0) || !std::isfinite(dev) || !std::isfinite(reach)) return false;
    // t of any point of the subtree <= kTNear / 4 (flatness, the origin's measured distance and that measurement's rounding: 4.1 u |o - p|_1),
    // Moller-Trumbore's error on it <= kTNear / 2 (16 u kappa (|o - p| + reach) / (0.75 |n . d|)); 1 % for the kernel's own fp32 evaluation
    const double u = std::ldexp(1.0, -24), tn = (double)kTNear;
    a0 = std::max(1.01 * (4.0 * dev + 2.0 * 16.0 * u * kappa * reach / 0.75) / tn, std::ldexp(1.0, -20));
    a2 = 1.01 * (4.0 * 4.1 * u + 2.0 * 16.0 * u * kappa / 0.75) / tn;
    return true;
}

namespace {
// rt_scene_check_bvh's part for the table: every entry that names a subtree is proven again from the tree as it is
bool check_skip_table(const HostScene& hs, std::string& err) {
    const size_t T = hs.wverts.size() / 9;
    if (hs.skip.empty()) return true; // (a scene description without triangles)
    if (hs.skip.size() != T) { err = "origin-skip table: one entry per triangle expected"; return false; }
    std::vector<uint8_t> is_word; // by node index: the node is some node's child (every reachable node but the root)
    is_word.assign(hs.nodes.size(), 0);
    for (const BvhNode& n : hs.nodes)
        for (int k = 0; k < 4; ++k)
            if (n.child[k] >= 0 && (size_t)n.child[k] < hs.nodes.size()) is_word[(size_t)n.child[k]] = 1;
    for (size_t t = 0; t < T; ++t) {
        const SkipRec& e = hs.skip[t];
        if (e.ref == kSkipNone) continue;
        const std::string at = "origin-skip entry of triangle " + std::to_string(t);
        const int32_t child = host_child_word(e.ref);
        if (child >= 0 && (device_child_word(child) != e.ref || (size_t)child >= hs.nodes.size() || !is_word[(size_t)child])) { err = at + ": not a child word"; return false; }
        std::vector<uint32_t> recs;
        if (!records_below(hs, child, 0, recs)) { err = at + ": names no subtree of at most " + std::to_string(kSkipMaxRecords) + " records"; return false; }
        bool member = false;
        for (uint32_t r : recs) member = member || hs.tris[r].global_index == t;
        if (!member) { err = at + ": the triangle is not in the subtree"; return false; }
        const float* w = &hs.wverts[9 * t];
        if (e.p[0] != w[0] || e.p[1] != w[1] || e.p[2] != w[2]) { err = at + ": p is not the triangle's first vertex"; return false; }
        double a0, a2;
        if (!skip_bounds(hs, e.n, e.p, child, a0, a2)) { err = at + ": the subtree is not coplanar with the triangle"; return false; }
        if (!((double)half_value((uint16_t)(e.a & 0xffffu)) >= a0) || !((double)half_value((uint16_t)(e.a >> 16)) >= a2) || !(a0 < 1.0)) {
            err = at + ": thresholds below what the subtree's flatness proves";
            return false;
        }
    }
    return true;
}
} // namespace

int check_bvh(const HostScene& hs, std::string& err) {
    const size_t T = hs.wverts.size() / 9;
    if (hs.nodes.empty()) { err = "no root node"; return RT_ERR_INVALID; }
    std::vector<uint32_t> seen(T, 0);
    // pre-split trees (scene_build.cpp: presplit): a triangle may sit in several leaves, each with the box of its pieces there
    const bool split = hs.rec_lo.size() == 3 * hs.tris.size() && hs.rec_hi.size() == 3 * hs.tris.size() && hs.n_split_triangles > 0;
    std::vector<std::vector<uint32_t>> pieces(split ? T : 0);
    size_t visited = 0;
    auto fail = [&](const std::string& m) { err = m; return false; };
    auto enter = [&](int32_t child, uint32_t depth) { // everything the walk is about to read
        if (depth >= (uint32_t)kStackSize) return fail("tree deeper than traversal stack");
        if (child >= 0) {
            if ((size_t)child >= hs.nodes.size()) return fail("child index out of range");
            if (++visited > hs.nodes.size()) return fail("cycle in node graph");
            return true;
        }
        const LeafRange leaf = leaf_range(child);
        if ((size_t)leaf.first + leaf.count > hs.tris.size()) return fail("leaf range out of bounds");
        for (uint32_t k = 0; k < leaf.count; ++k) {
            const TriRec& tr = hs.tris[leaf.first + k];
            if (tr.global_index >= T) return fail("leaf triangle has bad global index");
            for (uint32_t j = 0; j < k; ++j)
                if (hs.tris[leaf.first + j].global_index == tr.global_index) return fail("triangle twice in one leaf");
            if (seen[tr.global_index]++ && !split) return fail("triangle appears in two leaves");
            const float* w = &hs.wverts[9 * (size_t)tr.global_index];
            if (tr.v0[0] != w[0] || tr.v0[1] != w[1] || tr.v0[2] != w[2]) return fail("leaf triangle data mismatch");
            if (split) pieces[tr.global_index].push_back(leaf.first + k);
        }
        return true;
    };
    auto contained = [&](int32_t node, int k, const Box3& c) { // the decoded box must contain the subtree with at least half the builder's pad to spare
        const Box3 d = child_box(hs.nodes[(size_t)node], k);
        for (int a = 0; a < 3; ++a)
            if (!(d.lo[a] <= c.lo[a] - 0.5f * hs.pad) || !(d.hi[a] >= c.hi[a] + 0.5f * hs.pad))
                return fail("decoded child box does not contain its subtree (node " + std::to_string(node) + ")");
        return true;
    };
    Box3 all;
    if (!exact_boxes(hs, 0, 0, all, enter, contained)) return RT_ERR_INVALID;
    for (size_t t = 0; t < T; ++t)
        if (!seen[t]) { err = "triangle " + std::to_string(t) + " is in no leaf"; return RT_ERR_INVALID; }
    if (split) { // the pieces of a split triangle must cover it: every point of a barycentric grid lies in the box of one of its records
        for (size_t t = 0; t < T; ++t) {
            if (pieces[t].size() < 2) continue;
            const float* w = &hs.wverts[9 * t];
            for (int i = 0; i <= 8; ++i)
                for (int j = 0; i + j <= 8; ++j) {
                    const double u = i / 8.0, v = j / 8.0, ww = 1.0 - u - v;
                    double p[3];
                    for (int a = 0; a < 3; ++a) p[a] = ww * w[a] + u * w[3 + a] + v * w[6 + a];
                    bool in = false;
                    for (uint32_t rec : pieces[t]) {
                        bool inside = true;
                        for (int a = 0; a < 3; ++a) {
                            const double tol = 1e-6 * (std::fabs(p[a]) + 1.0);
                            inside = inside && p[a] >= (double)hs.rec_lo[3 * (size_t)rec + a] - tol && p[a] <= (double)hs.rec_hi[3 * (size_t)rec + a] + tol;
                        }
                        in = in || inside;
                    }
                    if (!in) { err = "the pieces of split triangle " + std::to_string(t) + " do not cover it"; return RT_ERR_INVALID; }
                }
        }
    }
    if (!check_skip_table(hs, err)) return RT_ERR_INVALID;
    return RT_OK;
}

// ---- what the host walks share ---------------------------------------------------------------------------------------------------------------
namespace {

// The walk every diagnostic below makes, from the root: inner(cur) visits the inner node cur, stacks the children to come back to and
// either descends (sets cur to the child, returns true) or not; leaf(range) tests a leaf's records. No second look at a popped child.
template <class Inner, class Leaf>
void walk_tree(std::vector<int32_t>& stack, uint64_t& visits, Inner&& inner, Leaf&& leaf) {
    stack.clear();
    int32_t cur = 0;
    for (;;) {
        if (cur >= 0) {
            visits++;
            if (inner(cur)) continue;
        } else {
            leaf(leaf_range(cur));
        }
        if (stack.empty()) break;
        cur = stack.back(), stack.pop_back();
    }
}

// The point traversal's inner step (rt_closest_step.h: closest_inner): the decoded child planes, the kernel's cull rule (closest_enters)
// against `best`, its sorting network on (lb, child) with +inf for a child not entered, the others stacked far to near.
inline bool point_inner(const BvhNode& nd, const float p[3], float best, std::vector<int32_t>& stack, int32_t& cur) {
    const float inf = std::numeric_limits<float>::infinity();
    float key[4];
    int32_t ch[4];
    for (int k = 0; k < 4; ++k) {
        ch[k] = nd.child[k], key[k] = inf;
        if (nd.child[k] == kChildEmpty) continue; // (its inverted box gives a finite lb: the word is what says it is absent)
        float lb = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const float lo = child_plane(nd, k, a, 0), hi = child_plane(nd, k, a, 1);
            const float e = std::max(std::max(lo - p[a], p[a] - hi), 0.0f);
            lb = std::fma(e, e, lb);
        }
        if (closest_enters(lb, best)) key[k] = std::min(lb, std::numeric_limits<float>::max()); // (an lb that overflowed is still a key)
    }
    auto ce = [&](int a, int b) { if (key[b] < key[a]) std::swap(key[a], key[b]), std::swap(ch[a], ch[b]); };
    ce(0, 1), ce(2, 3), ce(0, 2), ce(1, 3), ce(1, 2);
    for (int k = 3; k >= 1; --k)
        if (key[k] < inf) stack.push_back(ch[k]);
    if (key[0] < inf) cur = ch[0];
    return key[0] < inf;
}

// The ray traversal's inner step: the slab test of every child's box, box_of(k), against `bound` — a box AT the bound stays: a tie at a
// lower index is behind it — nearest child first, the others stacked. A child whose device word is `skip` counts as missed (the origin
// skip; kSkipNone: none).
inline void ray_inverse(const float d[3], float inv[3]) {
    for (int a = 0; a < 3; ++a) inv[a] = 1.0f / (std::fabs(d[a]) < 1e-30f ? std::copysign(1e-30f, d[a]) : d[a]);
}
template <class BoxOf>
bool ray_inner(const BvhNode& nd, const float o[3], const float inv[3], float bound, uint32_t skip, BoxOf&& box_of, std::vector<int32_t>& stack, int32_t& cur) {
    float key[4];
    int32_t ch[4];
    int m = 0;
    for (int k = 0; k < 4; ++k) {
        if (nd.child[k] == kChildEmpty || device_child_word(nd.child[k]) == skip) continue;
        const Box3 b = box_of(k);
        float tn = 0.0f, tf = bound;
        for (int a = 0; a < 3; ++a) {
            const float t0 = (b.lo[a] - o[a]) * inv[a], t1 = (b.hi[a] - o[a]) * inv[a];
            tn = std::max(tn, std::min(t0, t1)), tf = std::min(tf, std::max(t0, t1));
        }
        if (tn <= tf) key[m] = tn, ch[m] = nd.child[k], m++;
    }
    for (int a = 1; a < m; ++a) // nearest first
        for (int b = a; b > 0 && key[b] < key[b - 1]; --b) std::swap(key[b], key[b - 1]), std::swap(ch[b], ch[b - 1]);
    for (int a = m - 1; a >= 1; --a) stack.push_back(ch[a]);
    if (m) cur = ch[0];
    return m != 0;
}

// The sorted keyed list of nearest_host and multihit_host: entries (t, u, v, tri) in ascending (t, tri) order, t being a ray's t or a
// point's dist2. A candidate COUNTS iff t <= limit (a NaN t never does) and it lies behind the key, (t, tri) > (key_t, key_tri). The
// brute force adds every counting candidate, sorts and keeps the first k; the walk offers candidates to a list of at most k against the
// BOUND: (limit, kNoTri) while the list has free slots, (t, tri) of its k-th entry once it is full.
struct ListHit {
    float t, u, v;
    uint32_t tri;
};
inline bool hit_before(float t, uint32_t tri, float bt, uint32_t btri) { return t < bt || (t == bt && tri < btri); }
struct KeyedList {
    const size_t k;
    float limit = 0.0f, key_t = 0.0f, bound = 0.0f;
    uint32_t key_tri = 0u, bound_tri = kNoTri;
    std::vector<ListHit> hits;
    explicit KeyedList(size_t slots) : k(slots) {}

    // entry i's list: limit[i] or +inf, the key (key_t[i], key_tri[i]) or none, (-inf, 0)
    void open(uint32_t i, const float* limits, const float* key_ts, const uint32_t* key_tris) {
        const float inf = std::numeric_limits<float>::infinity();
        limit = limits ? limits[i] : inf, key_t = key_ts ? key_ts[i] : -inf, key_tri = key_ts ? key_tris[i] : 0u;
        bound = limit, bound_tri = kNoTri;
        hits.clear();
    }
    bool counts(const ListHit& c) const { return c.t <= limit && (c.t > key_t || (c.t == key_t && c.tri > key_tri)); }
    void add(const ListHit& c) { // the brute force
        if (counts(c)) hits.push_back(c);
    }
    void first_k() {
        std::stable_sort(hits.begin(), hits.end(), [](const ListHit& a, const ListHit& b) { return hit_before(a.t, a.tri, b.t, b.tri); });
        if (hits.size() > k) hits.resize(k);
    }
    // the walk: taken iff it sorts before the bound, counts and is not in the list already (a pre-split triangle sits in several leaves)
    void offer(const ListHit& c) {
        if (!hit_before(c.t, c.tri, bound, bound_tri) || !counts(c)) return;
        size_t at = 0;
        bool listed = false;
        for (const ListHit& h : hits) listed = listed || h.tri == c.tri, at += hit_before(h.t, h.tri, c.t, c.tri) ? 1 : 0;
        if (listed) return;
        hits.insert(hits.begin() + (ptrdiff_t)at, c);
        if (hits.size() > k) hits.pop_back();
        if (hits.size() == k) bound = hits.back().t, bound_tri = hits.back().tri;
    }
    // entry i's k output slots; the slots past the count hold the miss
    void store(uint32_t i, float* t_out, float* u_out, float* v_out, uint32_t* tri_out, uint32_t* count_out) const {
        if (count_out) count_out[i] = (uint32_t)hits.size();
        for (size_t s = 0; s < k; ++s) {
            const bool hit = s < hits.size();
            const size_t at = (size_t)i * k + s;
            if (t_out) t_out[at] = hit ? hits[s].t : std::numeric_limits<float>::infinity();
            if (u_out) u_out[at] = hit ? hits[s].u : 0.0f;
            if (v_out) v_out[at] = hit ? hits[s].v : 0.0f;
            if (tri_out) tri_out[at] = hit ? hits[s].tri : kNoTri;
        }
    }
};
// what both list walks refuse, `key` being the name of the key's first half
bool list_args_ok(uint32_t k, const float* key_t, const uint32_t* key_tri, const char* key, int use_bvh, const HostScene& hs, std::string& err) {
    if (use_bvh != 0 && use_bvh != 1) err = "use_bvh: 0 brute force, 1 the kernel's walk";
    else if (k < 1) err = "k must be at least 1";
    else if (!key_t != !key_tri) err = std::string("a resume key is ") + key + " and after_tri, both or neither";
    else if (use_bvh && hs.nodes.empty()) err = "no tree";
    return err.empty();
}
// triangle j of hs.wverts as the records hold it: v0, e1 = v1 - v0, e2 = v2 - v0
struct WorldTri {
    const float* v0;
    float e1[3], e2[3];
    explicit WorldTri(const float* w) : v0(w), e1{w[3] - w[0], w[4] - w[1], w[5] - w[2]}, e2{w[6] - w[0], w[7] - w[1], w[8] - w[2]} {}
};

} // namespace

// ---- node visits of a closest-hit walk on the host (rt_scene_count_visits) --------------------------------------------------------------------
// The walk the traversal kernels make — children entered nearest first, the others stacked, everything beyond the closest hit so far culled —
// with a choice of the child boxes it tests:
//   mode 0  the decoded quantised boxes, as the kernels test them
//   mode 1  the exact bounds of each child's subtree, padded as the builder pads them: what an unquantised (fp32) node would hold
//   mode 2  the exact padded bounds re-quantised on the node's grid with 2 more bits per plane (step / 4)
//   mode 4  mode 0 with the origin skip as the render kernels apply it (rt_bounce.h: origin_skip, the same fp32 expressions): tri_out holds ON
//           ENTRY the triangle every ray starts on (kNoTri: none), and the child whose word is that triangle's SkipRec::ref counts as missed
//           for a ray that passes the entry's test
//           (4, not 3: the modes 0..2 choose the BOXES, this one adds a cull to mode 0's boxes — bit 2 on top of box mode 0 — and 3 stays refused, as
//           callers and tests/test_host.py know it)
// so that the share of the visits that is the price of 8-bit planes can be read off. Counts only: no result of a
// render depends on it.
int count_visits(const HostScene& hs, uint32_t n, const float* org, const float* dir, int mode, uint64_t* node_visits, uint64_t* tri_tests, float* t_out,
                 uint32_t* tri_out, std::string& err) {
    if (mode != 4 && (mode < 0 || mode > 2)) { err = "mode: 0 quantised, 1 exact, 2 quantised with two more bits, 4 quantised with the origin skip"; return RT_ERR_INVALID; }
    const bool skipping = mode == 4;
    if (skipping) {
        mode = 0;
        if (!tri_out) { err = "mode 4: tri holds the triangle every ray starts on"; return RT_ERR_INVALID; }
        for (uint32_t i = 0; i < n; ++i)
            if (tri_out[i] != kNoTri && tri_out[i] >= hs.skip.size()) { err = "mode 4: start triangle out of range"; return RT_ERR_INVALID; }
    }
    if (hs.nodes.empty()) { err = "no tree"; return RT_ERR_INVALID; }
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<Box3> box(hs.nodes.size() * 4); // the box tested for child k of node i
    auto tested = [&](int32_t node, int k, const Box3& c) {
        const BvhNode& nd = hs.nodes[(size_t)node];
        Box3& out = box[(size_t)node * 4 + k];
        if (mode == 0) out = child_box(nd, k);
        else for (int a = 0; a < 3; ++a) {
            if (mode == 1) {
                out.lo[a] = c.lo[a] - hs.pad, out.hi[a] = c.hi[a] + hs.pad;
            } else {
                const float q = nd.scale(a) * 0.25f;
                out.lo[a] = nd.origin[a] + std::floor((c.lo[a] - hs.pad - nd.origin[a]) / q) * q;
                out.hi[a] = nd.origin[a] + std::ceil((c.hi[a] + hs.pad - nd.origin[a]) / q) * q;
            }
        }
        return true;
    };
    Box3 all;
    (void)exact_boxes(hs, 0, 0, all, [](int32_t, uint32_t) { return true; }, tested);
    uint64_t visits = 0, tests = 0;
    std::vector<int32_t> stack;
    for (uint32_t i = 0; i < n; ++i) {
        const float o[3] = {org[3 * i], org[3 * i + 1], org[3 * i + 2]}, d[3] = {dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]};
        float inv[3];
        ray_inverse(d, inv);
        float best = inf;
        uint32_t best_tri = kNoTri;
        uint32_t skip = kSkipNone;
        if (skipping && tri_out[i] != kNoTri) skip = origin_skip_word(hs.skip[tri_out[i]], o, d);
        walk_tree(stack, visits,
                  [&](int32_t& cur) {
                      const Box3* b = &box[(size_t)cur * 4];
                      return ray_inner(hs.nodes[(size_t)cur], o, inv, best, skip, [&](int k) { return b[k]; }, stack, cur);
                  },
                  [&](const LeafRange& leaf) {
                      for (uint32_t k = 0; k < leaf.count; ++k) {
                          tests++;
                          const TriRec& tr = hs.tris[leaf.first + k];
                          // Moller-Trumbore on (v0, e1, e2), in double: only the count matters here
                          const double e1[3] = {tr.e1[0], tr.e1[1], tr.e1[2]}, e2[3] = {tr.e2[0], tr.e2[1], tr.e2[2]};
                          const double p[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
                          const double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
                          if (det == 0.0) continue;
                          const double tv[3] = {o[0] - tr.v0[0], o[1] - tr.v0[1], o[2] - tr.v0[2]};
                          const double u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) / det;
                          const double q[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
                          const double v = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) / det;
                          if (u < 0.0 || v < 0.0 || u + v > 1.0) continue;
                          const double t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det;
                          if (t > (double)kTNear && (t < best || (t == best && tr.global_index < best_tri))) best = (float)t, best_tri = tr.global_index;
                      }
                  });
        if (t_out) t_out[i] = best;
        if (tri_out) tri_out[i] = best_tri;
    }
    if (node_visits) *node_visits = visits;
    if (tri_tests) *tri_tests = tests;
    return RT_OK;
}

// ---- closest-point queries on the host (rt_scene_closest_host; rt_closest_point.h) -------------------------------------------------------
// use_bvh = 0: the brute force over hs.tris with the contract's one text — a pre-split triangle's records all give the same candidate, so
// the leaf-ordered array stands for the triangle list. use_bvh = 1: the walk k_closest makes (rt_closest.hip) — the decoded child boxes, the
// kernel's cull rule (closest_enters), its sorting network on (lb, child) with +inf for a child not entered, the others stacked far to near,
// no second look at a popped child — counting node visits and triangle tests. Entries are not refused here: a NaN max_dist2 is a miss.
int closest_host(const HostScene& hs, uint32_t n, const float* pos, const float* max_dist2, int use_bvh, float* dist2_out, float* u_out, float* v_out,
                 uint32_t* tri_out, float* point_out, uint64_t* node_visits, uint64_t* tri_tests, std::string& err) {
    if (use_bvh != 0 && use_bvh != 1) { err = "use_bvh: 0 brute force, 1 the kernel's walk"; return RT_ERR_INVALID; }
    if (use_bvh && hs.nodes.empty()) { err = "no tree"; return RT_ERR_INVALID; }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    uint64_t visits = 0, tests = 0;
    std::vector<int32_t> stack;
    for (uint32_t i = 0; i < n; ++i) {
        const float p[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
        float best = max_dist2 ? max_dist2[i] : inf;
        uint32_t best_tri = kNoTri;
        ClosestPoint win{inf, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
        auto test = [&](const TriRec& tr) {
            tests++;
            const ClosestPoint c = closest_point_on_record(p, tr.v0, tr.e1, tr.e2);
            if (closest_better(c.dist2, tr.global_index, best, best_tri)) best = c.dist2, best_tri = tr.global_index, win = c;
        };
        if (!use_bvh) {
            for (const TriRec& tr : hs.tris) test(tr);
        } else {
            walk_tree(stack, visits, [&](int32_t& cur) { return point_inner(hs.nodes[(size_t)cur], p, best, stack, cur); },
                      [&](const LeafRange& leaf) {
                          for (uint32_t k = 0; k < leaf.count; ++k) test(hs.tris[leaf.first + k]);
                      });
        }
        const bool hit = best_tri != kNoTri;
        if (dist2_out) dist2_out[i] = hit ? best : inf;
        if (u_out) u_out[i] = hit ? win.u : 0.0f;
        if (v_out) v_out[i] = hit ? win.v : 0.0f;
        if (tri_out) tri_out[i] = best_tri;
        if (point_out)
            for (int a = 0; a < 3; ++a) point_out[3 * (size_t)i + a] = hit ? p[a] - win.r[a] : nan;
    }
    if (node_visits) *node_visits = visits;
    if (tri_tests) *tri_tests = tests;
    return RT_OK;
}

// ---- k-nearest closest-point queries on the host (rt_scene_nearest_host; include/rt_mi355x.h: rt_nearest_query) ----------------------------
// A candidate (rt_closest_point.h's one text) COUNTS iff dist2 <= max_dist2 and, with a key, (dist2, tri) > (after_dist2, after_tri); a NaN
// dist2 never counts. The answer is the k first counting candidates in (dist2, tri) order, every triangle once. use_bvh = 0: every
// triangle of hs.wverts in index order (e1 = v1 - v0, e2 = v2 - v0, as the records hold them), all counting candidates sorted, the first k.
// use_bvh = 1: the walk k_nearest makes — closest_host's inner step (the decoded child boxes, closest_enters, the sorting network, the
// others stacked far to near) against the BOUND, which is (max_dist2, kNoTri) while the list has free slots and (dist2, tri) of its k-th
// entry once it is full; a leaf's candidate is taken iff it passes closest_better against the bound, passes the key and is not in the list
// already (a pre-split triangle sits in several leaves) — counting node visits and triangle tests. k is any number >= 1 here (a list
// longer than a point's counting triangles never fills: the walk with the bound held at max_dist2). Entries are not refused: a NaN
// max_dist2 or key counts nothing.
int nearest_host(const HostScene& hs, uint32_t n, uint32_t k, const float* pos, const float* max_dist2, const float* after_dist2,
                 const uint32_t* after_tri, int use_bvh, float* dist2_out, float* u_out, float* v_out, uint32_t* tri_out, uint32_t* count_out,
                 uint64_t* node_visits, uint64_t* tri_tests, std::string& err) {
    if (!list_args_ok(k, after_dist2, after_tri, "after_dist2", use_bvh, hs, err)) return RT_ERR_INVALID;
    const size_t T = hs.wverts.size() / 9;
    uint64_t visits = 0, tests = 0;
    KeyedList list(k);
    std::vector<int32_t> stack;
    for (uint32_t i = 0; i < n; ++i) {
        const float p[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
        list.open(i, max_dist2, after_dist2, after_tri);
        auto candidate = [&](const float v0[3], const float e1[3], const float e2[3], uint32_t tri) {
            tests++;
            const ClosestPoint c = closest_point_on_record(p, v0, e1, e2);
            return ListHit{c.dist2, c.u, c.v, tri};
        };
        if (!use_bvh) {
            for (size_t j = 0; j < T; ++j) {
                const WorldTri w(&hs.wverts[9 * j]);
                list.add(candidate(w.v0, w.e1, w.e2, (uint32_t)j));
            }
            list.first_k();
        } else {
            walk_tree(stack, visits, [&](int32_t& cur) { return point_inner(hs.nodes[(size_t)cur], p, list.bound, stack, cur); },
                      [&](const LeafRange& leaf) {
                          for (uint32_t r = 0; r < leaf.count; ++r) {
                              const TriRec& tr = hs.tris[leaf.first + r];
                              list.offer(candidate(tr.v0, tr.e1, tr.e2, tr.global_index));
                          }
                      });
        }
        list.store(i, dist2_out, u_out, v_out, tri_out, count_out);
    }
    if (node_visits) *node_visits = visits;
    if (tri_tests) *tri_tests = tests;
    return RT_OK;
}

// ---- multi-hit ray queries on the host (rt_scene_multihit_host; include/rt_mi355x.h: rt_multihit_query) -------------------------------------
namespace {
inline float dot_f(const float a[3], const float b[3]) { return std::fma(a[2], b[2], std::fma(a[1], b[1], a[0] * b[0])); }
inline void cross_f(const float a[3], const float b[3], float r[3]) {
    r[0] = std::fma(a[1], b[2], -(a[2] * b[1])), r[1] = std::fma(a[2], b[0], -(a[0] * b[2])), r[2] = std::fma(a[0], b[1], -(a[1] * b[0]));
}
// The candidate of one triangle (v0, e1, e2) for a ray: R5's test as rt_device.h: tri_test_regs states it for the kernels — the fused
// cross and dot products, the edge tests on the numerators, inv = RN(1 / det), t > kTNear. false: no candidate.
inline bool ray_candidate(const float v0[3], const float e1[3], const float e2[3], const float o[3], const float d[3], ListHit& c) {
    float p[3], q[3];
    cross_f(d, e2, p);
    const float det = dot_f(e1, p);
    if (!(det != 0.0f)) return false;
    const float tv[3] = {o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]};
    cross_f(tv, e1, q);
    const float sgn = det < 0.0f ? -1.0f : 1.0f;
    const float un0 = dot_f(tv, p), vn0 = dot_f(d, q);
    const float un = un0 * sgn, vn = vn0 * sgn;
    if (!(un >= 0.0f && vn >= 0.0f && un + vn <= std::fabs(det))) return false;
    const float inv = 1.0f / det;
    const float t = dot_f(e2, q) * inv;
    if (!(t > kTNear)) return false;
    c.t = t, c.u = un0 * inv, c.v = vn0 * inv;
    return true;
}
} // namespace

// A candidate COUNTS iff kTNear < t <= tmax and, with a key, (t, tri) > (after_t, after_tri); the answer is the k first counting
// candidates in (t, tri) order, every triangle once. use_bvh = 0: every triangle of hs.wverts in index order (e1 = v1 - v0, e2 = v2 - v0, as
// the records hold them), all counting candidates sorted, the first k. use_bvh = 1: the walk k_multihit makes — the decoded child boxes
// culled against the BOUND and kept at equal distance, nearest child first; the bound is (tmax, kNoTri) while the list has free slots
// and (t, tri) of its k-th entry once it is full; a leaf's candidate is taken iff it sorts before the bound, passes the key and is not
// in the list already (a pre-split triangle sits in several leaves) — counting node visits and triangle tests. k is any number >= 1
// here (a list longer than a ray's hits never fills: the walk with the bound held at tmax). Rays are not refused: a NaN tmax or key
// counts nothing.
int multihit_host(const HostScene& hs, uint32_t n, uint32_t k, const float* org, const float* dir, const float* tmax, const float* after_t,
                  const uint32_t* after_tri, int use_bvh, float* t_out, float* u_out, float* v_out, uint32_t* tri_out, uint32_t* count_out,
                  uint64_t* node_visits, uint64_t* tri_tests, std::string& err) {
    if (!list_args_ok(k, after_t, after_tri, "after_t", use_bvh, hs, err)) return RT_ERR_INVALID;
    const size_t T = hs.wverts.size() / 9;
    uint64_t visits = 0, tests = 0;
    KeyedList list(k);
    std::vector<int32_t> stack;
    for (uint32_t i = 0; i < n; ++i) {
        const float o[3] = {org[3 * (size_t)i], org[3 * (size_t)i + 1], org[3 * (size_t)i + 2]};
        const float d[3] = {dir[3 * (size_t)i], dir[3 * (size_t)i + 1], dir[3 * (size_t)i + 2]};
        list.open(i, tmax, after_t, after_tri);
        if (!use_bvh) {
            for (size_t j = 0; j < T; ++j) {
                const WorldTri w(&hs.wverts[9 * j]);
                ListHit c{0.0f, 0.0f, 0.0f, (uint32_t)j};
                tests++;
                if (ray_candidate(w.v0, w.e1, w.e2, o, d, c)) list.add(c);
            }
            list.first_k();
        } else {
            float inv[3];
            ray_inverse(d, inv);
            walk_tree(stack, visits,
                      [&](int32_t& cur) {
                          const BvhNode& nd = hs.nodes[(size_t)cur];
                          return ray_inner(nd, o, inv, list.bound, kSkipNone, [&](int c) { return child_box(nd, c); }, stack, cur);
                      },
                      [&](const LeafRange& leaf) {
                          for (uint32_t r = 0; r < leaf.count; ++r) {
                              const TriRec& tr = hs.tris[leaf.first + r];
                              ListHit c{0.0f, 0.0f, 0.0f, tr.global_index};
                              tests++;
                              if (ray_candidate(tr.v0, tr.e1, tr.e2, o, d, c)) list.offer(c);
                          }
                      });
        }
        list.store(i, t_out, u_out, v_out, tri_out, count_out);
    }
    if (node_visits) *node_visits = visits;
    if (tri_tests) *tri_tests = tests;
    return RT_OK;
}

// ---- occlusion gathers on the host (rt_scene_occlusion_host; include/rt_mi355x.h: rt_occlusion_query) ---------------------------------------
namespace {
// XorShift32State and random_unit_vector as rt_device.h states them (rng_next, rng_range, rng_unit_vector), one fp32 operation each
inline float host_rng_next(uint32_t& a) {
    uint32_t x = a;
    x ^= x << 13, x ^= x >> 17, x ^= x << 5;
    a = x;
    return (float)x * (1.0f / 4294967296.0f);
}
inline float host_rng_range(uint32_t& a, float mn, float mx) { return mn + (mx - mn) * host_rng_next(a); }
} // namespace

// The contract's loop per entry: per sample the three draws, d = normal + u, the DEGENERATE test on l2, w = d * (1 / sqrt(l2)) and one
// any-hit query on (pos, w, max_dist). A candidate COUNTS iff kTNear < t <= max_dist (ray_candidate above, multihit_host's). use_bvh = 0:
// every triangle of hs.wverts in index order, occluded iff one counts. use_bvh = 1: the walk k_occlusion_gather makes — the decoded child
// boxes culled against max_dist and kept at equal distance, nearest child first, a leaf tested whole, the walk over at the first leaf with
// a counting candidate — counting node visits and triangle tests. Entries are not refused: a NaN max_dist occludes nothing, a normal that
// is not finite makes every sample degenerate.
int occlusion_host(const HostScene& hs, uint32_t n, uint32_t samples, const float* pos, const float* normal, const float* max_dist, const uint32_t* rng,
                   int use_bvh, uint32_t* rng_out, float* visibility, float* bent, uint32_t* clear_out, uint32_t* rays_out, uint64_t* node_visits,
                   uint64_t* tri_tests, std::string& err) {
    if (use_bvh != 0 && use_bvh != 1) { err = "use_bvh: 0 brute force, 1 the kernel's walk"; return RT_ERR_INVALID; }
    if (samples < 1 || samples > RT_OCCLUSION_MAX_SAMPLES) { err = "samples must be 1 .. " + std::to_string(RT_OCCLUSION_MAX_SAMPLES); return RT_ERR_INVALID; }
    if (use_bvh && hs.nodes.empty()) { err = "no tree"; return RT_ERR_INVALID; }
    const float inf = std::numeric_limits<float>::infinity();
    const size_t T = hs.wverts.size() / 9;
    uint64_t visits = 0, tests = 0;
    std::vector<int32_t> stack;
    for (uint32_t i = 0; i < n; ++i) {
        const float* o = pos + 3 * (size_t)i;
        const float* nr = normal + 3 * (size_t)i;
        const float md = max_dist ? max_dist[i] : inf;
        uint32_t a = rng[i], clear = 0, rays = 0;
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t s = 0; s < samples; ++s) {
            float u[3];
            for (int k = 0; k < 3; ++k) u[k] = host_rng_range(a, -1.0f, 1.0f);
            const float ui = 1.0f / std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
            const float d[3] = {nr[0] + u[0] * ui, nr[1] + u[1] * ui, nr[2] + u[2] * ui};
            const float l2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            if (!(l2 > 0.0f) || !(l2 < inf)) { // DEGENERATE: no ray
                clear++;
                continue;
            }
            const float wi = 1.0f / std::sqrt(l2);
            const float w[3] = {d[0] * wi, d[1] * wi, d[2] * wi};
            rays++;
            bool occluded = false;
            ListHit c{0.0f, 0.0f, 0.0f, 0u};
            if (!use_bvh) {
                for (size_t j = 0; j < T && !occluded; ++j) {
                    const WorldTri t(&hs.wverts[9 * j]);
                    tests++;
                    occluded = ray_candidate(t.v0, t.e1, t.e2, o, w, c) && c.t <= md;
                }
            } else {
                float inv[3];
                ray_inverse(w, inv);
                walk_tree(stack, visits,
                          [&](int32_t& cur) {
                              const BvhNode& nd = hs.nodes[(size_t)cur];
                              return ray_inner(nd, o, inv, md, kSkipNone, [&](int k) { return child_box(nd, k); }, stack, cur);
                          },
                          [&](const LeafRange& leaf) {
                              for (uint32_t r = 0; r < leaf.count; ++r) {
                                  const TriRec& tr = hs.tris[leaf.first + r];
                                  tests++;
                                  if (ray_candidate(tr.v0, tr.e1, tr.e2, o, w, c) && c.t <= md) occluded = true;
                              }
                              if (occluded) stack.clear(); // ANY: the walk is over
                          });
            }
            if (!occluded) {
                clear++;
                for (int k = 0; k < 3; ++k) sum[k] = sum[k] + w[k];
            }
        }
        const float fs = (float)samples;
        if (visibility) visibility[i] = (float)clear / fs;
        if (bent)
            for (int k = 0; k < 3; ++k) bent[3 * (size_t)i + k] = sum[k] / fs;
        if (clear_out) clear_out[i] = clear;
        if (rays_out) rays_out[i] = rays;
        if (rng_out) rng_out[i] = a;
    }
    if (node_visits) *node_visits = visits;
    if (tri_tests) *tri_tests = tests;
    return RT_OK;
}

} // namespace rt
