// scene_build.cpp — host side of rt_scene_create: validation, instance flattening, BVH build.
//
// Replaces what Embree does behind rtcCommitScene for the reference (src/scene.cpp:101-107,
// 406-439,487-507): a two-level instanced triangle BVH becomes ONE flattened world-space BVH2
// over all instance triangles. The image does not depend on the tree (closest t, ties to the
// lowest global triangle index), so the builder is free to optimise for traversal speed.
//
// Compiled with -ffp-contract=off: the world-space vertices and edges computed here are part of
// the arithmetic contract shared with the CPU oracle (instance transform row order, e1 = v1 - v0).
// The diagnostics of a built scene (costs, check_bvh, count_visits) are in scene_check.cpp.
#include "scene_build.h"
#include "bvh_quantise.h"
#include "scene_rules.h"
#include "rt_knobs.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <deque>
#include <queue>

namespace rt {
namespace {

struct GNode { // generic build node
    float lo[3], hi[3];
    int32_t left = -1, right = -1; // inner: both >= 0
    uint32_t first = 0, count = 0; // range in `order`
    uint32_t depth = 0;
};

// The builders work on REFERENCES: (triangle, box). Without pre-splitting there is one reference per triangle and its box is the
// triangle's; presplit() below replaces large triangles by several references with the boxes of the triangle's clipped pieces.
struct Builder {
    const std::vector<float>& wv; // 9 per triangle
    std::vector<uint32_t> order;   // reference ids, partitioned in place by the builders
    std::vector<GNode> nodes;
    std::vector<float> cent; // 3 per reference
    std::vector<float> tlo, thi; // per-reference boxes
    std::vector<uint32_t> ref_tri; // reference -> triangle
    uint32_t n_split = 0;          // triangles that were split

    explicit Builder(const std::vector<float>& w) : wv(w) {
        const size_t n = w.size() / 9;
        order.resize(n);
        cent.resize(3 * n);
        tlo.resize(3 * n);
        thi.resize(3 * n);
        ref_tri.resize(n);
        for (size_t t = 0; t < n; ++t) {
            order[t] = (uint32_t)t;
            ref_tri[t] = (uint32_t)t;
            for (int a = 0; a < 3; ++a) {
                float p0 = w[9 * t + a], p1 = w[9 * t + 3 + a], p2 = w[9 * t + 6 + a];
                tlo[3 * t + a] = std::min(p0, std::min(p1, p2));
                thi[3 * t + a] = std::max(p0, std::max(p1, p2));
                cent[3 * t + a] = 0.5f * (tlo[3 * t + a] + thi[3 * t + a]);
            }
        }
    }

    void range_bounds(uint32_t first, uint32_t count, float* lo, float* hi, float* clo, float* chi) const {
        for (int a = 0; a < 3; ++a) {
            lo[a] = clo[a] = std::numeric_limits<float>::infinity();
            hi[a] = chi[a] = -std::numeric_limits<float>::infinity();
        }
        for (uint32_t k = 0; k < count; ++k) {
            uint32_t t = order[first + k];
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], tlo[3 * t + a]);
                hi[a] = std::max(hi[a], thi[3 * t + a]);
                clo[a] = std::min(clo[a], cent[3 * t + a]);
                chi[a] = std::max(chi[a], cent[3 * t + a]);
            }
        }
    }
};

// ---- spatial pre-splitting of large triangles (early split clipping with a budget) ------------------------------------
// A triangle that is large against the nodes it ends up in drags their boxes over empty space (a wall made of two triangles, Sponza's
// floor): every ray through that space pays a node visit and a triangle test for nothing. Its remedy in a top-down builder is the spatial
// split (Stich et al. 2009); the form built here is the pre-pass of Ernst & Greiner 2007 with a budget, as production builders use it:
// the references with the FATTEST boxes (most enclosed volume) are cut at the spatial median of their longest axis — the triangle is clipped against the plane
// (Sutherland-Hodgman, in double), each piece gets the tight box of its polygon — until the budget of extra references is spent or
// nothing is left above the floor size. The tree is then built over the pieces; a leaf stores the TRIANGLE (each once per leaf).
// A triangle in several leaves cannot change a result: the closest hit is min t with ties to the lowest triangle index (rule R5),
// and testing the same triangle twice yields the same t. What it costs: more leaf records; what it buys: tighter boxes.
struct SplitRef {
    uint32_t tri;
    int n;            // polygon vertices
    double p[10][3];  // a triangle clipped by k axis-aligned planes has at most 3 + k vertices; pieces are cut at most ~7 times
    float lo[3], hi[3];
    float key;        // fatness of the box (below): what the heap orders by
};
struct SplitRefLess {
    bool operator()(const SplitRef* a, const SplitRef* b) const { return a->key < b->key; }
};

// What makes a reference worth splitting is the EMPTY VOLUME its box encloses, not its size: a wall of two axis-aligned triangles has a
// flat box that drags nothing along (and is cheaper to trace than a tessellated one), a large triangle that runs diagonally through space
// has a fat one. Key: the geometric mean of the box's three extents (0 for a flat box).
inline float fatness(const float* lo, const float* hi) {
    const float dx = std::max(hi[0] - lo[0], 0.0f), dy = std::max(hi[1] - lo[1], 0.0f), dz = std::max(hi[2] - lo[2], 0.0f);
    return std::cbrt(dx * dy * dz);
}

inline void poly_box(SplitRef& r, const float* plo, const float* phi) { // tight box of the polygon, rounded outward, inside the parent's
    for (int a = 0; a < 3; ++a) {
        double lo = r.p[0][a], hi = r.p[0][a];
        for (int i = 1; i < r.n; ++i) lo = std::min(lo, r.p[i][a]), hi = std::max(hi, r.p[i][a]);
        float flo = (float)lo, fhi = (float)hi;
        if ((double)flo > lo) flo = std::nextafter(flo, -INFINITY);
        if ((double)fhi < hi) fhi = std::nextafter(fhi, INFINITY);
        r.lo[a] = std::max(flo, plo[a]), r.hi[a] = std::min(fhi, phi[a]);
    }
    r.key = fatness(r.lo, r.hi);
}

// polygon `in` clipped to the half space (keep_below ? x[axis] <= pos : x[axis] >= pos)
inline int clip_poly(const double (*in)[3], int n, int axis, double pos, bool keep_below, double (*out)[3]) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const double* a = in[i];
        const double* b = in[(i + 1) % n];
        const double da = keep_below ? pos - a[axis] : a[axis] - pos, db = keep_below ? pos - b[axis] : b[axis] - pos;
        if (da >= 0.0) {
            if (m < 10) std::memcpy(out[m++], a, sizeof(double) * 3);
        }
        if ((da > 0.0 && db < 0.0) || (da < 0.0 && db > 0.0)) {
            const double t = da / (da - db);
            if (m < 10) {
                for (int k = 0; k < 3; ++k) out[m][k] = a[k] + t * (b[k] - a[k]);
                out[m][axis] = pos;
                ++m;
            }
        }
    }
    return m;
}

// budget: extra references as a fraction of the triangle count; floor_extent: boxes whose fatness is below this are left alone
void presplit(Builder& b, double budget, float floor_extent) {
    const size_t T = b.wv.size() / 9;
    const size_t max_refs = T + (size_t)((double)T * budget);
    if (T == 0 || max_refs == T) return;
    std::deque<SplitRef> pool; // stable addresses
    std::priority_queue<SplitRef*, std::vector<SplitRef*>, SplitRefLess> heap;
    std::vector<uint8_t> was_split(T, 0);
    for (size_t t = 0; t < T; ++t) {
        const float ext = fatness(&b.tlo[3 * t], &b.thi[3 * t]);
        if (!(ext > floor_extent)) continue;
        pool.emplace_back();
        SplitRef& r = pool.back();
        r.tri = (uint32_t)t, r.n = 3;
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) r.p[v][a] = (double)b.wv[9 * t + 3 * v + a];
        std::memcpy(r.lo, &b.tlo[3 * t], 12), std::memcpy(r.hi, &b.thi[3 * t], 12);
        r.key = ext;
        heap.push(&r);
    }
    if (heap.empty()) return;
    size_t n_refs = T;
    std::vector<const SplitRef*> done; // pieces that are final
    while (!heap.empty()) {
        SplitRef* r = heap.top();
        heap.pop();
        if (n_refs >= max_refs || !(r->key > floor_extent) || r->n >= 9) {
            done.push_back(r);
            continue;
        }
        int axis = 0;
        for (int a = 1; a < 3; ++a)
            if (r->hi[a] - r->lo[a] > r->hi[axis] - r->lo[axis]) axis = a;
        const double pos = 0.5 * ((double)r->lo[axis] + (double)r->hi[axis]);
        pool.emplace_back();
        SplitRef& l = pool.back();
        pool.emplace_back();
        SplitRef& h = pool.back();
        l.tri = h.tri = r->tri;
        l.n = clip_poly(r->p, r->n, axis, pos, true, l.p);
        h.n = clip_poly(r->p, r->n, axis, pos, false, h.p);
        if (l.n < 3 || h.n < 3) { // the plane does not cut the polygon (degenerate): leave the piece as it is
            r->n = 9;             // (never asked again)
            done.push_back(r);
            continue;
        }
        float llo[3], lhi[3], hlo[3], hhi[3];
        std::memcpy(llo, r->lo, 12), std::memcpy(lhi, r->hi, 12), std::memcpy(hlo, r->lo, 12), std::memcpy(hhi, r->hi, 12);
        lhi[axis] = std::nextafter((float)pos, INFINITY), hlo[axis] = std::nextafter((float)pos, -INFINITY);
        poly_box(l, llo, lhi), poly_box(h, hlo, hhi);
        was_split[r->tri] = 1;
        ++n_refs;
        heap.push(&l), heap.push(&h);
    }
    // the reference arrays: unsplit triangles keep their slot; the pieces of split triangles are appended (the first piece takes the slot)
    std::vector<uint8_t> slot_used(T, 0);
    for (const SplitRef* r : done) {
        if (!was_split[r->tri]) continue; // popped but never cut: the triangle's own reference stands
        size_t id;
        if (!slot_used[r->tri]) id = r->tri, slot_used[r->tri] = 1;
        else {
            id = b.ref_tri.size();
            b.ref_tri.push_back(r->tri);
            b.order.push_back((uint32_t)id);
            b.tlo.resize(3 * (id + 1)), b.thi.resize(3 * (id + 1)), b.cent.resize(3 * (id + 1));
        }
        for (int a = 0; a < 3; ++a) b.tlo[3 * id + a] = r->lo[a], b.thi[3 * id + a] = r->hi[a], b.cent[3 * id + a] = 0.5f * (r->lo[a] + r->hi[a]);
    }
    for (size_t t = 0; t < T; ++t) b.n_split += was_split[t];
}

// ---- what the two top-down builders share: the to-do stack of index ranges ---------------------------------------------------------------------
struct Work {
    int32_t node;
    uint32_t first, count, depth;
};
std::vector<Work> start_tree(Builder& b) { // the root over every reference
    b.nodes.assign(1, GNode{});
    return {{0, 0, (uint32_t)b.order.size(), 0}};
}
// makes nd an inner node over w's range cut at `split`: two fresh nodes, their ranges on the stack
void open_children(Builder& b, GNode& nd, const Work& w, uint32_t split, std::vector<Work>& todo) {
    nd.left = (int32_t)b.nodes.size();
    nd.right = nd.left + 1;
    b.nodes.push_back(GNode{});
    b.nodes.push_back(GNode{});
    todo.push_back({nd.left, w.first, split, w.depth + 1});
    todo.push_back({nd.right, w.first + split, w.count - split, w.depth + 1});
}

// ---- LBVH: 63-bit Morton order + top-down split at the highest differing bit -----------------------
inline uint64_t expand21(uint64_t v) { // spread the low 21 bits to every third bit
    v &= 0x1fffffull;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}

void build_lbvh(Builder& b) {
    const uint32_t n = (uint32_t)b.order.size();
    float lo[3], hi[3], clo[3], chi[3];
    b.range_bounds(0, n, lo, hi, clo, chi);
    std::vector<std::pair<uint64_t, uint32_t>> keys(n);
    for (uint32_t t = 0; t < n; ++t) {
        uint64_t code = 0;
        for (int a = 0; a < 3; ++a) {
            double ext = (double)chi[a] - (double)clo[a];
            double f = ext > 0 ? ((double)b.cent[3 * t + a] - (double)clo[a]) / ext : 0.0;
            uint64_t q = (uint64_t)std::min(2097151.0, std::max(0.0, f * 2097152.0));
            code |= expand21(q) << (2 - a);
        }
        keys[t] = {code, t};
    }
    std::sort(keys.begin(), keys.end());
    for (uint32_t i = 0; i < n; ++i) b.order[i] = keys[i].second;

    std::vector<Work> todo = start_tree(b);
    while (!todo.empty()) {
        Work w = todo.back();
        todo.pop_back();
        GNode nd;
        float c0[3], c1[3];
        b.range_bounds(w.first, w.count, nd.lo, nd.hi, c0, c1);
        nd.first = w.first, nd.count = w.count, nd.depth = w.depth;
        if (w.count > (uint32_t)kMaxLeafTris) {
            uint64_t ka = keys[w.first].first, kb = keys[w.first + w.count - 1].first;
            uint32_t split;
            if (ka == kb || w.depth >= 56) {
                split = w.count / 2; // identical codes (or runaway depth): halve the index range
            } else {
                int bit = 63 - __builtin_clzll(ka ^ kb);
                uint64_t mask = 1ull << bit;
                // first element whose `bit` is set (codes share all higher bits, so it is monotone)
                uint32_t l = 0, r = w.count;
                while (l < r) {
                    uint32_t m = (l + r) / 2;
                    if (keys[w.first + m].first & mask) r = m; else l = m + 1;
                }
                split = l;
                if (split == 0 || split == w.count) split = w.count / 2;
            }
            open_children(b, nd, w, split, todo);
        }
        b.nodes[w.node] = nd;
    }
}

// ---- binned SAH, top-down -------------------------------------------------------------------------
void build_sah(Builder& b, uint32_t max_sah_depth, float trav_cost) {
    constexpr int NB = 32;
    std::vector<Work> todo = start_tree(b);
    std::vector<uint32_t> tmp;
    while (!todo.empty()) {
        Work w = todo.back();
        todo.pop_back();
        GNode nd;
        float clo[3], chi[3];
        b.range_bounds(w.first, w.count, nd.lo, nd.hi, clo, chi);
        nd.first = w.first, nd.count = w.count, nd.depth = w.depth;
        bool make_leaf = w.count == 1;
        uint32_t split = 0;
        if (!make_leaf) {
            const float parent_area = half_area(nd.lo, nd.hi);
            float best_cost = std::numeric_limits<float>::infinity();
            int best_axis = -1, best_bin = -1;
            if (w.depth < max_sah_depth) {
                for (int a = 0; a < 3; ++a) {
                    float ext = chi[a] - clo[a];
                    if (!(ext > 0.0f)) continue;
                    float scale = (float)NB / ext;
                    uint32_t cnt[NB] = {0};
                    float blo[NB][3], bhi[NB][3];
                    for (int i = 0; i < NB; ++i)
                        for (int k = 0; k < 3; ++k) blo[i][k] = INFINITY, bhi[i][k] = -INFINITY;
                    for (uint32_t k = 0; k < w.count; ++k) {
                        uint32_t t = b.order[w.first + k];
                        int bi = std::min(NB - 1, std::max(0, (int)((b.cent[3 * t + a] - clo[a]) * scale)));
                        cnt[bi]++;
                        for (int j = 0; j < 3; ++j) {
                            blo[bi][j] = std::min(blo[bi][j], b.tlo[3 * t + j]);
                            bhi[bi][j] = std::max(bhi[bi][j], b.thi[3 * t + j]);
                        }
                    }
                    float ra[NB];
                    uint32_t rc[NB];
                    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                    uint32_t c = 0;
                    for (int i = NB - 1; i > 0; --i) {
                        c += cnt[i];
                        for (int j = 0; j < 3; ++j) lo[j] = std::min(lo[j], blo[i][j]), hi[j] = std::max(hi[j], bhi[i][j]);
                        ra[i] = half_area(lo, hi), rc[i] = c;
                    }
                    for (int j = 0; j < 3; ++j) lo[j] = INFINITY, hi[j] = -INFINITY;
                    c = 0;
                    for (int i = 0; i < NB - 1; ++i) {
                        c += cnt[i];
                        for (int j = 0; j < 3; ++j) lo[j] = std::min(lo[j], blo[i][j]), hi[j] = std::max(hi[j], bhi[i][j]);
                        if (c == 0 || rc[i + 1] == 0) continue;
                        float cost = half_area(lo, hi) * (float)c + ra[i + 1] * (float)rc[i + 1];
                        if (cost < best_cost) best_cost = cost, best_axis = a, best_bin = i;
                    }
                }
            }
            // leaf cost = count * area; split cost = 1 traversal step * area + children
            if (w.count <= (uint32_t)kMaxLeafTris &&
                !(best_axis >= 0 && best_cost + trav_cost * parent_area < (float)w.count * parent_area)) {
                make_leaf = true;
            } else if (best_axis >= 0) {
                float ext = chi[best_axis] - clo[best_axis];
                float scale = (float)NB / ext;
                auto mid = std::partition(b.order.begin() + w.first, b.order.begin() + w.first + w.count, [&](uint32_t t) {
                    int bi = std::min(NB - 1, std::max(0, (int)((b.cent[3 * t + best_axis] - clo[best_axis]) * scale)));
                    return bi <= best_bin;
                });
                split = (uint32_t)(mid - (b.order.begin() + w.first));
            }
            if (!make_leaf && (split == 0 || split == w.count)) {
                // all centroids coincide (or depth guard): median split on the index order
                split = w.count / 2;
                std::nth_element(b.order.begin() + w.first, b.order.begin() + w.first + split,
                                 b.order.begin() + w.first + w.count);
            }
        }
        if (!make_leaf) open_children(b, nd, w, split, todo);
        b.nodes[w.node] = nd;
    }
}

// ---- insertion-based optimisation of the binary tree (after Bittner, Hapala, Havran 2013) ---------------------
// A top-down SAH build decides every split greedily and never revisits it. This pass takes inner nodes in order of
// decreasing surface area, unlinks the node (its two subtrees become orphans, its parent is replaced by its
// sibling) and re-inserts both subtrees where they increase the tree's total surface area least, found by a
// branch-and-bound search from the root. Leaves (triangle ranges) are untouched: only the topology above them
// changes, so the traversal result cannot change, only the number of nodes a ray visits.
void optimise_by_reinsertion(Builder& b, int passes, double fraction) {
    std::vector<GNode>& n = b.nodes;
    const int32_t count = (int32_t)n.size();
    if (count < 7) return;
    std::vector<int32_t> parent((size_t)count, -1);
    for (int32_t i = 0; i < count; ++i)
        if (n[i].left >= 0) parent[n[i].left] = i, parent[n[i].right] = i;
    auto area = [&](int32_t i) { return half_area(n[i].lo, n[i].hi); };
    auto merge = [&](int32_t dst, int32_t a, int32_t c) {
        for (int k = 0; k < 3; ++k) n[dst].lo[k] = std::min(n[a].lo[k], n[c].lo[k]), n[dst].hi[k] = std::max(n[a].hi[k], n[c].hi[k]);
    };
    auto refit_up = [&](int32_t i) {
        for (; i >= 0; i = parent[i]) {
            float lo[3], hi[3];
            for (int k = 0; k < 3; ++k)
                lo[k] = std::min(n[n[i].left].lo[k], n[n[i].right].lo[k]), hi[k] = std::max(n[n[i].left].hi[k], n[n[i].right].hi[k]);
            if (std::memcmp(lo, n[i].lo, 12) == 0 && std::memcmp(hi, n[i].hi, 12) == 0) break;
            std::memcpy(n[i].lo, lo, 12), std::memcpy(n[i].hi, hi, 12);
        }
    };
    auto union_area = [&](int32_t a, int32_t c) {
        float lo[3], hi[3];
        for (int k = 0; k < 3; ++k) lo[k] = std::min(n[a].lo[k], n[c].lo[k]), hi[k] = std::max(n[a].hi[k], n[c].hi[k]);
        return half_area(lo, hi);
    };
    struct Cand { float bound; int32_t node; float induced; };
    auto cmp = [](const Cand& x, const Cand& y) { return x.bound > y.bound; };
    std::vector<Cand> heap;
    // the node below which `x` costs least: cost = area(node ∪ x) + the growth of every ancestor of the new parent
    auto find_best = [&](int32_t x) {
        const float ax = area(x);
        float best = std::numeric_limits<float>::infinity();
        int32_t best_node = -1;
        heap.clear();
        for (int32_t c : {n[0].left, n[0].right}) heap.push_back({0.0f, c, 0.0f}); // never AT the root: node 0 stays the root
        std::make_heap(heap.begin(), heap.end(), cmp);
        while (!heap.empty()) {
            std::pop_heap(heap.begin(), heap.end(), cmp);
            const Cand c = heap.back();
            heap.pop_back();
            if (c.bound >= best) break;
            const float direct = union_area(c.node, x);
            const float total = c.induced + direct;
            if (total < best) best = total, best_node = c.node;
            const float child_induced = total - area(c.node);
            if (n[c.node].left >= 0 && child_induced + ax < best) {
                heap.push_back({child_induced + ax, n[c.node].left, child_induced});
                std::push_heap(heap.begin(), heap.end(), cmp);
                heap.push_back({child_induced + ax, n[c.node].right, child_induced});
                std::push_heap(heap.begin(), heap.end(), cmp);
            }
        }
        return best_node;
    };
    std::vector<int32_t> order;
    for (int pass = 0; pass < passes; ++pass) {
        order.clear();
        for (int32_t i = 1; i < count; ++i)
            if (n[i].left >= 0 && parent[i] > 0) order.push_back(i); // inner, not the root, not a child of the root
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t c) { return area(a) > area(c); });
        order.resize((size_t)((double)order.size() * fraction));
        for (int32_t N : order) {
            const int32_t P = parent[N];
            if (n[N].left < 0 || P <= 0) continue; // the tree changed under us: N became a root child or was recycled
            const int32_t G = parent[P];
            const int32_t S = n[P].left == N ? n[P].right : n[P].left;
            int32_t X[2] = {n[N].left, n[N].right};
            if (area(X[0]) < area(X[1])) std::swap(X[0], X[1]);
            // unlink N and P: G adopts S
            (n[G].left == P ? n[G].left : n[G].right) = S;
            parent[S] = G;
            refit_up(G);
            int32_t spare[2] = {P, N};
            for (int k = 0; k < 2; ++k) {
                const int32_t x = X[k], F = spare[k];
                const int32_t B = find_best(x);
                const int32_t PB = parent[B];
                (n[PB].left == B ? n[PB].left : n[PB].right) = F;
                parent[F] = PB;
                n[F].left = B, n[F].right = x, n[F].first = 0, n[F].count = 0;
                parent[B] = F, parent[x] = F;
                merge(F, B, x);
                refit_up(PB);
            }
        }
    }
    // depths (statistics only) from the new topology
    std::vector<int32_t> stack{0};
    n[0].depth = 0;
    while (!stack.empty()) {
        const int32_t i = stack.back();
        stack.pop_back();
        if (n[i].left >= 0) {
            n[n[i].left].depth = n[n[i].right].depth = n[i].depth + 1;
            stack.push_back(n[i].left), stack.push_back(n[i].right);
        }
    }
}

// ---- collapse to four children -----------------------------------------------------------------------------------------------------------------
// Which binary nodes become BVH4 nodes: dynamic programme over the binary tree (after Ylitie, Karras, Laine 2017).
// best[n][k] = least SAH cost of covering subtree n with at most k child slots of its BVH4 parent; a subtree that
// takes one slot is a leaf or a BVH4 node of its own (area + the best way to hand its 4 slots to its two halves).
// cut[n][4] = slots a BVH4 node n gives to its LEFT half. best[0][1] / area(root) is the 4-wide tree's surface-area cost.
struct Collapse {
    std::vector<std::array<float, 5>> best;
    std::vector<std::array<uint8_t, 5>> cut;
};

void collapse_dp(const Builder& b, Collapse& c) {
    c.best.assign(b.nodes.size(), {}), c.cut.assign(b.nodes.size(), {});
    std::vector<int32_t> post, st{0};
    while (!st.empty()) { // pre-order, reversed = children before parents
        const int32_t i = st.back();
        st.pop_back();
        post.push_back(i);
        if (b.nodes[i].left >= 0) st.push_back(b.nodes[i].left), st.push_back(b.nodes[i].right);
    }
    for (size_t q = post.size(); q-- > 0;) {
        const int32_t i = post[q];
        const GNode& g = b.nodes[i];
        const float ar = half_area(g.lo, g.hi);
        if (g.left < 0) {
            for (int k = 1; k <= 4; ++k) c.best[i][k] = ar * (float)g.count;
            continue;
        }
        float dist[5];
        uint8_t dl[5];
        for (int k = 2; k <= 4; ++k) {
            dist[k] = std::numeric_limits<float>::infinity(), dl[k] = 1;
            for (int l = 1; l < k; ++l) {
                const float cost = c.best[g.left][l] + c.best[g.right][k - l];
                if (cost < dist[k]) dist[k] = cost, dl[k] = (uint8_t)l;
            }
        }
        c.best[i][1] = ar + dist[4];
        for (int k = 2; k <= 4; ++k) c.best[i][k] = std::min(dist[k], c.best[i][k - 1]);
        c.cut[i][4] = dl[4]; // what the node does with its OWN four slots when it is a BVH4 node (best[i][1])
    }
}

// the children subtree n contributes to a BVH4 node that grants it up to k slots: the recorded decisions, expanded
void gather(const Builder& b, const Collapse& c, int32_t n, int k, int32_t* kids, int& nk) {
    const GNode& g = b.nodes[n];
    if (k <= 1 || g.left < 0) { kids[nk++] = n; return; }
    // as a PARENT's subtree with k slots: either distribute them or fall back to k-1
    float dist = std::numeric_limits<float>::infinity();
    int dl = 1;
    for (int l = 1; l < k; ++l) {
        const float cost = c.best[g.left][l] + c.best[g.right][k - l];
        if (cost < dist) dist = cost, dl = l;
    }
    if (dist < c.best[n][k - 1]) gather(b, c, g.left, dl, kids, nk), gather(b, c, g.right, k - dl, kids, nk);
    else gather(b, c, n, k - 1, kids, nk);
}

// the up to four children of the BVH4 node made of binary node n; greedy (RT_BVH_COLLAPSE=greedy): open the inner child with the largest surface area
int wide_children(const Builder& b, const Collapse& c, bool use_dp, int32_t n, int32_t* kids) {
    const GNode& g = b.nodes[n];
    int nk = 0;
    if (use_dp) {
        const int li = c.cut[n][4];
        gather(b, c, g.left, li, kids, nk), gather(b, c, g.right, 4 - li, kids, nk);
        return nk;
    }
    kids[nk++] = g.left, kids[nk++] = g.right;
    while (nk < 4) {
        int best = -1;
        float best_area = -1.0f;
        for (int k = 0; k < nk; ++k) {
            const GNode& ch = b.nodes[kids[k]];
            const float ar = ch.left >= 0 ? half_area(ch.lo, ch.hi) : -1.0f;
            if (ar > best_area) best_area = ar, best = k;
        }
        if (best < 0) break;
        const GNode& ch = b.nodes[kids[best]];
        kids[best] = ch.left;
        kids[nk++] = ch.right;
    }
    return nk;
}

// ---- the binary tree of one builder kind -------------------------------------------------------------------------------------------------------
// The builders' knobs (developer build), read once per scene.
struct BuildOptions {
    // pre-splitting of large triangles (SAH builder only): at most 30 % more references, only boxes FATTER (geometric mean of the three
    // extents) than 1/64 of the scene's largest extent — the finely tessellated bench scene has none and neither have axis-aligned walls
    // (their trees are unchanged); large triangles that cross space diagonally do. RT_BVH_SPLIT_BUDGET=0 switches it off,
    // RT_BVH_SPLIT_FLOOR=<fraction of the scene extent> moves the floor.
    double budget = 0.3, floor_frac = 1.0 / 64.0;
    // one pass over the larger half of the inner nodes: -2.6 % SAH cost, 17.9 -> 17.5 node visits per ray on the
    // atrium (+0.7 % rays/s) for 0.18 s of extra build time; further passes change nothing. RT_BVH_REINSERT=0: off
    int passes = 1;
    double fraction = 0.5;
    float trav_cost = 1.0f; // cost of one traversal step relative to one triangle test, for the leaf-vs-split decision of small ranges
    bool use_dp = true;     // RT_BVH_COLLAPSE=greedy restores the open-the-largest-child rule

    BuildOptions() {
        if (const char* e = dev_knob("RT_BVH_SPLIT_BUDGET")) budget = std::max(0.0, std::min(4.0, std::atof(e)));
        if (const char* e = dev_knob("RT_BVH_SPLIT_FLOOR")) floor_frac = std::max(1e-4, std::min(1.0, std::atof(e)));
        if (const char* e = dev_knob("RT_BVH_REINSERT")) passes = std::atoi(e);
        if (const char* e = dev_knob("RT_BVH_REINSERT_FRACTION")) fraction = std::atof(e);
        if (const char* e = dev_knob("RT_SAH_TRAV_COST")) trav_cost = (float)std::atof(e);
        if (const char* e = dev_knob("RT_BVH_COLLAPSE")) use_dp = std::string(e) != "greedy";
    }
};

// Where pre-splitting did split, the tree without splits is built too and the one with the lower surface-area cost of its 4-wide collapse
// is kept (a 116-triangle Cornell box gets worse, a tilted hall 15 % better).
std::unique_ptr<Builder> build_binary(int kind, const HostScene& hs, const BuildOptions& o) {
    std::unique_ptr<Builder> bp(new Builder(hs.wverts));
    if (kind == RT_BVH_LBVH || kind == RT_BVH_LBVH_GPU) { // (a GPU request for fewer than 8 triangles: the host LBVH)
        build_lbvh(*bp);
        return bp;
    }
    const bool balanced = kind == RT_BVH_MEDIAN_INTERNAL;
    float ext = 0.0f;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, hs.bounds_hi[a] - hs.bounds_lo[a]);
    auto run = [&](Builder& b, bool split) {
        if (split && !balanced && o.budget > 0.0) presplit(b, o.budget, (float)(o.floor_frac * (double)ext));
        build_sah(b, balanced ? 0u : 48u, o.trav_cost);
        if (!balanced && o.passes > 0) optimise_by_reinsertion(b, o.passes, std::min(1.0, std::max(0.0, o.fraction)));
    };
    auto wide_cost = [](const Builder& b) {
        Collapse c;
        collapse_dp(b, c);
        return (double)c.best[0][1] / std::max(1e-30, (double)half_area(b.nodes[0].lo, b.nodes[0].hi));
    };
    run(*bp, true);
    if (bp->n_split > 0) {
        std::unique_ptr<Builder> plain(new Builder(hs.wverts));
        run(*plain, false);
        if (bp->nodes[0].left < 0 || plain->nodes[0].left < 0 || wide_cost(*plain) <= wide_cost(*bp)) bp = std::move(plain);
    }
    return bp;
}

// ---- emission: the 4-wide tree into hs.nodes / hs.tris -----------------------------------------------------------------------------------------
// the leaf records of binary leaf g: the triangles of its references, each once; a record keeps the box of its pieces HERE
int32_t emit_leaf(const Builder& b, const std::vector<TriRec>& gtris, const GNode& g, uint32_t depth, HostScene& hs) {
    const uint32_t first = (uint32_t)hs.tris.size();
    uint32_t count = 0;
    for (uint32_t k = 0; k < g.count; ++k) {
        const uint32_t ref = b.order[g.first + k], tri = b.ref_tri[ref];
        uint32_t at = count;
        for (uint32_t j = 0; j < count; ++j)
            if (hs.tris[first + j].global_index == tri) at = j;
        if (at == count) {
            hs.tris.push_back(gtris[tri]);
            for (int a = 0; a < 3; ++a) hs.rec_lo.push_back(b.tlo[3 * ref + a]), hs.rec_hi.push_back(b.thi[3 * ref + a]);
            ++count;
        } else {
            for (int a = 0; a < 3; ++a) {
                float& lo = hs.rec_lo[3 * (size_t)(first + at) + a];
                float& hi = hs.rec_hi[3 * (size_t)(first + at) + a];
                lo = std::min(lo, b.tlo[3 * ref + a]), hi = std::max(hi, b.thi[3 * ref + a]);
            }
        }
    }
    hs.max_leaf_tris = std::max(hs.max_leaf_tris, count);
    hs.max_depth = std::max(hs.max_depth, depth);
    return leaf_child(first, count);
}

// Collapses the binary tree into a 4-wide one and emits it top first. Emission order: largest surface area first until the LDS-staged top
// of the tree is complete (the first kTopNodes nodes of the array are the children of the nodes a ray is most likely to visit; level order
// staged 2 % fewer expected visits), depth-first below it, so that the nodes and the triangles of one subtree are contiguous in memory
// (fewer distinct cache lines per ray than a pure breadth-first layout). Returns false with err set; `single` tells a root that is one leaf.
bool emit_tree(const Builder& b, const std::vector<TriRec>& gtris, const BuildOptions& o, HostScene& hs, bool& single, std::string& err) {
    const GNode& g0 = b.nodes[0];
    hs.tris.reserve(b.order.size());
    hs.n_split_triangles = b.n_split;
    hs.nodes.push_back(empty_node());
    single = g0.left < 0;
    if (single) { // give the root one leaf child
        if (g0.count > (uint32_t)kMaxLeafTris) { err = "internal: oversized root leaf"; return false; }
        Box3 kb;
        std::memcpy(kb.lo, g0.lo, 12), std::memcpy(kb.hi, g0.hi, 12);
        if (!quantise_node(hs.nodes[0], 1, &kb, hs.pad)) { err = "internal: quantisation failed"; return false; }
        hs.nodes[0].child[0] = emit_leaf(b, gtris, g0, 1, hs);
        hs.sah_cost = (double)g0.count;
        return true;
    }
    const double root_area = std::max(1e-30, (double)half_area(g0.lo, g0.hi));
    double cost = 0.0;
    Collapse c;
    if (o.use_dp) collapse_dp(b, c);
    struct Item { int32_t gnode; int32_t slot; uint32_t depth; };
    std::deque<Item> q{{0, 0, 0}};
    while (!q.empty()) {
        Item it;
        if (hs.nodes.size() < (size_t)kTopNodes) { // the nodes the traversal kernels stage in LDS
            size_t pick = 0; // the pending node a ray is most likely to visit: the one with the largest surface area
            float best_area = -1.0f;
            for (size_t i = 0; i < q.size(); ++i) {
                const float ar = half_area(b.nodes[q[i].gnode].lo, b.nodes[q[i].gnode].hi);
                if (ar > best_area) best_area = ar, pick = i;
            }
            it = q[pick];
            q.erase(q.begin() + (std::ptrdiff_t)pick);
        } else { it = q.back(); q.pop_back(); }
        const GNode& g = b.nodes[it.gnode];
        cost += (double)half_area(g.lo, g.hi) / root_area;
        int32_t kids[4];
        const int nk = wide_children(b, c, o.use_dp, it.gnode, kids);
        BvhNode out = empty_node();
        Item pending[4];
        int n_pending = 0;
        Box3 kb[4];
        for (int k = 0; k < nk; ++k) std::memcpy(kb[k].lo, b.nodes[kids[k]].lo, 12), std::memcpy(kb[k].hi, b.nodes[kids[k]].hi, 12);
        if (!quantise_node(out, nk, kb, hs.pad)) { err = "internal: quantisation failed"; return false; }
        for (int k = 0; k < nk; ++k) {
            const GNode& ch = b.nodes[kids[k]];
            if (ch.left < 0) {
                if (ch.count == 0 || ch.count > (uint32_t)kMaxLeafTris) { err = "internal: bad leaf size"; return false; }
                out.child[k] = emit_leaf(b, gtris, ch, it.depth + 1, hs);
                cost += (double)half_area(ch.lo, ch.hi) / root_area * (double)ch.count;
            } else {
                out.child[k] = (int32_t)hs.nodes.size();
                hs.nodes.push_back(empty_node());
                pending[n_pending++] = {kids[k], out.child[k], it.depth + 1};
            }
        }
        // top phase: children in order at the back; depth-first phase: reversed, so child 0 is next
        if (hs.nodes.size() < (size_t)kTopNodes) for (int k = 0; k < n_pending; ++k) q.push_back(pending[k]);
        else for (int k = n_pending - 1; k >= 0; --k) q.push_back(pending[k]);
        hs.nodes[it.slot] = out;
    }
    hs.sah_cost = cost;
    if (const char* e = dev_knob("RT_BVH_VERBOSE")) { // diagnostic: leaves by size
        if (e[0] == '1') {
            size_t by[5] = {0, 0, 0, 0, 0};
            for (const BvhNode& n : hs.nodes)
                for (int k = 0; k < 4; ++k)
                    if (n.child[k] < 0 && n.child[k] != kChildEmpty) by[leaf_range(n.child[k]).count]++;
            std::fprintf(stderr, "[rt bvh] %zu nodes, leaves with 1 / 2 / 3 / 4 triangles: %zu / %zu / %zu / %zu, %zu records for %zu triangles (%u split)\n", hs.nodes.size(),
                         by[1], by[2], by[3], by[4], hs.tris.size(), gtris.size(), hs.n_split_triangles);
        }
    }
    if (hs.tris.size() < gtris.size() || hs.tris.size() > b.order.size()) { err = "internal: leaf record count mismatch after build"; return false; }
    return true;
}

// Exact worst-case traversal stack need: at every level all siblings of the entered child may be waiting.
uint32_t stack_need(const std::vector<BvhNode>& nodes, int32_t node) {
    const BvhNode& n = nodes[node];
    uint32_t nk = 0, worst = 0;
    for (int k = 0; k < 4; ++k) nk += n.child[k] != kChildEmpty;
    for (int k = 0; k < 4; ++k)
        if (n.child[k] != kChildEmpty) worst = std::max(worst, (nk - 1) + (n.child[k] >= 0 ? stack_need(nodes, n.child[k]) : 0u));
    return worst;
}

// One attempt at the tree, from clean tree fields: RT_OK, an error, or kTooDeep where the tree would overflow the traversal stack (or the
// device builder's emission loop) and the balanced builder has to take over.
constexpr int kTooDeep = -1000;
int build_tree(int kind, const std::vector<TriRec>& gtris, const BuildOptions& o, HostScene& hs, std::string& err) {
    hs.nodes.clear(), hs.tris.clear(), hs.rec_lo.clear(), hs.rec_hi.clear();
    hs.max_depth = hs.max_leaf_tris = hs.n_split_triangles = hs.stack_need = 0;
    hs.sah_cost = 0.0;
    const bool on_device = kind == RT_BVH_LBVH_GPU && gtris.size() >= 8; // whole build on the device (lbvh_gpu.hip); tiny scenes use the host
    if (on_device) {
        const int rc = build_lbvh_gpu(hs, gtris, err);
        if (rc == RT_ERR_UNSUPPORTED) return kTooDeep; // degenerate Morton order (deeper than the emission loop allows)
        if (rc != RT_OK) return rc;
    } else {
        bool single = false;
        if (!emit_tree(*build_binary(kind, hs, o), gtris, o, hs, single, err)) return RT_ERR_INVALID;
        if (single) return RT_OK; // (built_by and stack_need stay unset for a root that is one leaf)
    }
    hs.stack_need = stack_need(hs.nodes, 0);
    if (hs.stack_need + 2 >= (uint32_t)kStackSize) return kTooDeep;
    hs.built_by = (int8_t)(kind == RT_BVH_LBVH_GPU && !on_device ? RT_BVH_LBVH : kind);
    if (on_device) hs.sah_cost = decoded_sah_cost(hs);
    return RT_OK;
}

// ---- the stages before the tree ----------------------------------------------------------------------------------------------------------------
int validate_desc(const rt_scene_desc* d, int bvh_kind, std::string& err) {
    auto bad = [&](const char* m) { err = m; return (int)RT_ERR_INVALID; };
    if (!d) return bad("null scene description");
    if (d->n_triangles && (!d->positions || !d->normals || !d->uvs || !d->indices || !d->tri_instance)) return bad("null geometry array");
    if ((d->n_instances && !d->instances) || (d->n_materials && !d->materials)) return bad("null instance/material array");
    if (d->n_layers > RT_TEX_MAX_LAYERS) return bad("more than 128 texture layers");
    if (d->n_layers && !d->textures) return bad("null texture array");
    if (d->n_triangles >= (1u << 28)) return bad("too many triangles (limit 2^28)");
    if (bvh_kind != RT_BVH_DEFAULT && bvh_kind != RT_BVH_LBVH && bvh_kind != RT_BVH_SAH && bvh_kind != RT_BVH_MEDIAN_INTERNAL &&
        bvh_kind != RT_BVH_LBVH_GPU)
        return bad("unknown bvh_kind");
    for (uint32_t i = 0; i < d->n_instances; ++i)
        if (d->instances[i].material >= d->n_materials) return bad("instance material out of range");
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const rt_material& m = d->materials[i];
        if (m.type > RT_MAT_DIELECTRIC || m.tex_kind > RT_TEX_IMAGE) return bad("bad material type");
        if (m.tex_kind == RT_TEX_IMAGE && m.type != RT_MAT_DIELECTRIC && m.type != RT_MAT_NONE && m.tex_layer >= d->n_layers)
            return bad("material texture layer out of range");
    }
    for (uint32_t t = 0; t < d->n_triangles; ++t) {
        if (d->tri_instance[t] >= d->n_instances) return bad("tri_instance out of range");
        for (int k = 0; k < 3; ++k)
            if (d->indices[3 * t + k] >= d->n_vertices) return bad("vertex index out of range");
    }
    return RT_OK;
}

// sky, textures, the device's instance table (shading_rows; inst_slot[i]: instance i's row) and the materials
void fill_tables(const rt_scene_desc& d, HostScene& hs, std::vector<uint32_t>& inst_slot) {
    hs.sky[0] = d.sky[0], hs.sky[1] = d.sky[1], hs.sky[2] = d.sky[2];
    hs.n_layers = d.n_layers;
    if (d.n_layers) hs.tex.assign(d.textures, d.textures + (size_t)d.n_layers * 512u * 512u * 4u);
    hs.packed_mat = d.n_instances <= (1u << kPackedInstBits) && d.n_materials <= (1u << (32u - kPackedInstBits));
    std::vector<uint64_t> use(d.n_instances, 0);
    for (uint32_t t = 0; t < d.n_triangles; ++t) use[d.tri_instance[t]]++;
    shading_rows(d.instances, d.n_instances, use, hs.packed_mat, hs.inst, inst_slot);
    hs.mats.resize(d.n_materials);
    for (uint32_t i = 0; i < d.n_materials; ++i) {
        const rt_material& m = d.materials[i];
        MatRec& r = hs.mats[i];
        r.type = m.type, r.tex_kind = m.tex_kind, r.tex_layer = m.tex_layer;
        std::memcpy(r.color, m.color, 12), std::memcpy(r.emissive, m.emissive, 12);
        r.roughness = m.roughness, r.ior = m.ior, r.pad = 0;
    }
}

// world vertices, the triangle records in global order and the shading records (each rule: scene_rules.h)
void flatten(const rt_scene_desc& d, const std::vector<uint32_t>& inst_slot, HostScene& hs, std::vector<TriRec>& gtris) {
    const uint32_t T = d.n_triangles;
    world_vertices(T, d.indices, d.tri_instance, d.instances, d.positions, hs.wverts);
    hs.shade.resize(T);
    gtris.assign(T, TriRec{});
    for (uint32_t t = 0; t < T; ++t) {
        TriRec& tr = gtris[t];
        tri_record(&hs.wverts[9 * (size_t)t], tr.v0, tr.e1, tr.e2);
        tr.global_index = t;
        ShadeRec& s = hs.shade[t];
        const uint32_t ii = d.tri_instance[t], *idx = d.indices + 3 * (size_t)t;
        shade_normals(s, idx, d.normals);
        std::memcpy(s.uv0, d.uvs + 2 * idx[0], 8), std::memcpy(s.uv1, d.uvs + 2 * idx[1], 8);
        std::memcpy(s.uv2, d.uvs + 2 * idx[2], 8);
        s.instance = shading_word(hs.packed_mat, inst_slot[ii], d.instances[ii].material, ii);
    }
}

} // namespace

int build_host_scene(const rt_scene_desc* d, int bvh_kind, HostScene& hs, std::string& err) {
    if (const int rc = validate_desc(d, bvh_kind, err)) return rc;
    hs = HostScene{};
    std::vector<uint32_t> inst_slot;
    fill_tables(*d, hs, inst_slot);
    std::vector<TriRec> gtris;
    flatten(*d, inst_slot, hs, gtris);
    if (gtris.empty()) {
        hs.built_by = (int8_t)bvh_kind;
        hs.nodes.assign(1, empty_node());
        hs.tris.assign(1, TriRec{}); // one dummy record so device pointers are never null
        hs.tris[0].global_index = kNoTri;
        return RT_OK;
    }
    if (!world_bounds(hs.wverts, hs.bounds_lo, hs.bounds_hi, hs.pad, err)) return RT_ERR_INVALID;
    const BuildOptions options;
    for (int kind = bvh_kind;; kind = RT_BVH_MEDIAN_INTERNAL) { // the requested builder, then the balanced fallback
        const int rc = build_tree(kind, gtris, options, hs, err);
        if (rc != kTooDeep) return rc;
        if (kind == RT_BVH_MEDIAN_INTERNAL) { err = "internal: BVH deeper than the traversal stack"; return RT_ERR_INVALID; }
        err.clear();
    }
}

void world_vertices(uint32_t n_tris, const uint32_t* indices, const uint32_t* tri_instance, const rt_instance* inst, const float* positions,
                    std::vector<float>& wv) {
    wv.resize(9 * (size_t)n_tris);
    for (uint32_t t = 0; t < n_tris; ++t) {
        const float* m = inst[tri_instance[t]].transform;
        for (int k = 0; k < 3; ++k) {
            const uint32_t vi = indices[3 * (size_t)t + k];
            const float x = positions[3 * (size_t)vi], y = positions[3 * (size_t)vi + 1], z = positions[3 * (size_t)vi + 2];
            for (int a = 0; a < 3; ++a) wv[9 * (size_t)t + 3 * k + a] = world_coord(m, a, x, y, z);
        }
    }
}

bool world_bounds(const std::vector<float>& wv, float lo[3], float hi[3], float& pad, std::string& err) {
    for (float v : wv)
        if (!std::isfinite(v)) { err = "non-finite world-space vertex"; return false; }
    for (int a = 0; a < 3; ++a) lo[a] = INFINITY, hi[a] = -INFINITY;
    for (size_t i = 0; i < wv.size(); ++i) {
        const int a = (int)(i % 3);
        lo[a] = std::min(lo[a], wv[i]), hi[a] = std::max(hi[a], wv[i]);
    }
    return scene_padding(lo, hi, pad, err);
}

// The device's instance table. Packed shading word (the rule, rt_types.h): the material index travels in the word, so what is left of an
// instance is its normal matrix — and a scene has far fewer DISTINCT matrices than instances (one instance per glTF node and primitive:
// 166 and 5 on the atrium). The table holds every distinct bit pattern once, ordered by the number of triangles that use it, so that the
// head of the table — what the shading kernels stage in LDS — covers the most hits. slot[i]: instance i's row of the table.
void shading_rows(const rt_instance* inst, uint32_t n, const std::vector<uint64_t>& use, bool packed, std::vector<InstRec>& out,
                  std::vector<uint32_t>& slot) {
    slot.assign(n, 0);
    if (packed) {
        std::map<std::array<uint32_t, 9>, uint32_t> seen; // bit pattern -> provisional row
        std::vector<std::array<uint32_t, 9>> rows;
        std::vector<uint64_t> row_use;
        for (uint32_t i = 0; i < n; ++i) {
            std::array<uint32_t, 9> key;
            std::memcpy(key.data(), inst[i].normal_mat, 36);
            auto it = seen.find(key);
            if (it == seen.end()) {
                it = seen.emplace(key, (uint32_t)rows.size()).first;
                rows.push_back(key), row_use.push_back(0);
            }
            slot[i] = it->second;
            row_use[it->second] += use[i];
        }
        std::vector<uint32_t> order(rows.size()), rank(rows.size());
        for (uint32_t k = 0; k < order.size(); ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return row_use[a] > row_use[b]; });
        for (uint32_t k = 0; k < order.size(); ++k) rank[order[k]] = k;
        out.assign(rows.size(), InstRec{});
        for (uint32_t k = 0; k < rows.size(); ++k) std::memcpy(out[rank[k]].normal_mat, rows[k].data(), 36);
        for (uint32_t i = 0; i < n; ++i) slot[i] = rank[slot[i]];
    } else {
        out.assign(n, InstRec{});
        for (uint32_t i = 0; i < n; ++i) {
            std::memcpy(out[i].normal_mat, inst[i].normal_mat, sizeof(float) * 9);
            out[i].material = inst[i].material;
            slot[i] = i;
        }
    }
}

bool scene_padding(const float lo[3], const float hi[3], float& pad, std::string& err) {
    float ext = 0.0f, amax = 0.0f;
    for (int a = 0; a < 3; ++a) {
        ext = std::max(ext, hi[a] - lo[a]);
        amax = std::max(amax, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
    }
    // Absolute padding of every box: 2e-5 x scene scale. Float rounding of the slab test and of the
    // Moller-Trumbore t is ~1e-7 x scale, so a padded box can only cull triangles the exact test
    // would also miss ("culling is conservative").
    pad = 2e-5f * std::max(ext, amax) + 1e-30f;
    // Finite vertices can still span more than fp32 holds (x from -2e38 to 2e38): no builder can quantise such a scene, and every
    // builder refuses it here alike, before one is chosen (the device quantiser would otherwise meet it only per node).
    bool finite = std::isfinite(ext) && std::isfinite(pad);
    for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(lo[a] - pad) && std::isfinite(hi[a] + pad);
    if (!finite) { err = "scene extent overflows fp32 (the padded bounds are not finite)"; return false; }
    return true;
}

void node_levels(const std::vector<BvhNode>& nodes, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_start) {
    const size_t n = nodes.size();
    std::vector<uint32_t> height(n, 0), post;
    std::vector<uint32_t> st{0};
    post.reserve(n);
    while (!st.empty()) { // pre-order from the root, reversed below: children before parents
        const uint32_t i = st.back();
        st.pop_back();
        post.push_back(i);
        for (int k = 0; k < 4; ++k)
            if (nodes[i].child[k] >= 0) st.push_back((uint32_t)nodes[i].child[k]);
    }
    uint32_t top = 0;
    for (size_t q = post.size(); q-- > 0;) {
        const uint32_t i = post[q];
        uint32_t h = 0;
        for (int k = 0; k < 4; ++k)
            if (nodes[i].child[k] >= 0) h = std::max(h, height[(size_t)nodes[i].child[k]] + 1);
        height[i] = h, top = std::max(top, h);
    }
    level_start.assign((size_t)top + 2, 0);
    for (uint32_t i : post) level_start[(size_t)height[i] + 1]++;
    for (size_t h = 1; h < level_start.size(); ++h) level_start[h] += level_start[h - 1];
    level_nodes.assign(post.size(), 0);
    std::vector<uint32_t> at(level_start.begin(), level_start.end() - 1);
    // ascending node index within a level (nodes the root cannot reach — none in a built tree — are left out)
    std::vector<uint8_t> reached(n, 0);
    for (uint32_t i : post) reached[i] = 1;
    for (uint32_t i = 0; i < (uint32_t)n; ++i)
        if (reached[i]) level_nodes[at[height[i]]++] = i;
}

void record_boxes(HostScene& hs) {
    hs.rec_lo.assign(3 * hs.tris.size(), 0.0f), hs.rec_hi.assign(3 * hs.tris.size(), 0.0f);
    for (size_t r = 0; r < hs.tris.size(); ++r) {
        if (hs.tris[r].global_index == kNoTri) continue;
        const Box3 b = tri_box(&hs.wverts[9 * (size_t)hs.tris[r].global_index]);
        std::memcpy(&hs.rec_lo[3 * r], b.lo, 12), std::memcpy(&hs.rec_hi[3 * r], b.hi, 12);
    }
}

Box3 leaf_bounds(const HostScene& hs, int32_t child) {
    const bool split = hs.rec_lo.size() == 3 * hs.tris.size() && hs.rec_hi.size() == 3 * hs.tris.size() && hs.n_split_triangles > 0;
    const LeafRange leaf = leaf_range(child);
    Box3 b = empty_box();
    for (uint32_t r = leaf.first; r < leaf.first + leaf.count; ++r) {
        Box3 rb;
        if (split) std::memcpy(rb.lo, &hs.rec_lo[3 * (size_t)r], 12), std::memcpy(rb.hi, &hs.rec_hi[3 * (size_t)r], 12);
        else rb = tri_box(&hs.wverts[9 * (size_t)hs.tris[r].global_index]);
        grow(b, rb);
    }
    return b;
}

bool refit_host(HostScene& hs, const std::vector<uint32_t>& level_nodes, std::vector<float>& box, std::string& err) {
    // leaf records: the packed v0 / e1 / e2 of their triangle, and the whole triangle's box (a pre-split triangle's pieces mean nothing now)
    record_boxes(hs);
    for (TriRec& tr : hs.tris)
        if (tr.global_index != kNoTri) tri_record(&hs.wverts[9 * (size_t)tr.global_index], tr.v0, tr.e1, tr.e2);
    box.assign(6 * hs.nodes.size(), 0.0f);
    const auto inner_box = [&](int32_t child) { Box3 b; std::memcpy(&b, &box[6 * (size_t)child], sizeof(Box3)); return b; };
    const auto tri_of = [&](uint32_t r) { return &hs.wverts[9 * (size_t)hs.tris[r].global_index]; };
    for (uint32_t i : level_nodes) {
        Box3 u; BvhNode q;
        const RefitResult res = refit_node(hs.nodes[i], inner_box, tri_of, hs.pad, u, q);
        if (res == kRefitEmpty) continue; // the empty scene's root
        if (res == kRefitRefused) { err = "a refit node's child boxes could not be quantised"; return false; }
        std::memcpy(&box[6 * (size_t)i], &u, sizeof(Box3));
        hs.nodes[i] = q;
    }
    hs.sah_cost = refit_sah_cost(hs, box);
    return true;
}

// ---- the origin skip (rt_types.h: SkipRec) -------------------------------------------------------------------------------------------------------
void clear_skip_table(HostScene& hs) {
    SkipRec none{};
    none.ref = kSkipNone;
    hs.skip.assign(hs.wverts.size() / 9, none);
}

// Per triangle: its plane (unit normal in double, rounded to fp32; first vertex), then up from its leaf while skip_bounds proves the whole
// subtree flat on that plane — a subtree that fails makes every larger one fail, so the last one proven is the highest. A pre-split
// triangle starts from the first leaf that holds a piece of it (any subtree proven flat may be skipped, the triangle's own or not).
void build_skip_table(HostScene& hs) {
    clear_skip_table(hs);
    const size_t T = hs.skip.size();
    if (T == 0 || hs.nodes.empty()) return;
    std::vector<int32_t> parent(hs.nodes.size(), -1);    // node -> the node that names it
    std::vector<int32_t> rec_node(hs.tris.size(), -1);   // leaf record -> the node whose leaf child holds it
    std::vector<uint8_t> rec_slot(hs.tris.size(), 0);
    for (size_t i = 0; i < hs.nodes.size(); ++i)
        for (int k = 0; k < 4; ++k) {
            const int32_t c = hs.nodes[i].child[k];
            if (c == kChildEmpty) continue;
            if (c >= 0) {
                if ((size_t)c < hs.nodes.size()) parent[(size_t)c] = (int32_t)i;
                continue;
            }
            const LeafRange leaf = leaf_range(c);
            for (uint32_t r = leaf.first; r < leaf.first + leaf.count && r < hs.tris.size(); ++r) rec_node[r] = (int32_t)i, rec_slot[r] = (uint8_t)k;
        }
    std::vector<int32_t> first_rec(T, -1);
    for (size_t r = hs.tris.size(); r-- > 0;)
        if (hs.tris[r].global_index < T && rec_node[r] >= 0) first_rec[hs.tris[r].global_index] = (int32_t)r;
    for (size_t t = 0; t < T; ++t) {
        if (first_rec[t] < 0) continue;
        const float* w = &hs.wverts[9 * t];
        double e1[3], e2[3];
        for (int a = 0; a < 3; ++a) e1[a] = (double)w[3 + a] - (double)w[a], e2[a] = (double)w[6 + a] - (double)w[a];
        const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        if (!(len > 0.0) || !std::isfinite(len)) continue;
        SkipRec e{};
        for (int a = 0; a < 3; ++a) e.n[a] = (float)(c[a] / len), e.p[a] = w[a];
        int32_t at = rec_node[(size_t)first_rec[t]];
        int32_t child = hs.nodes[(size_t)at].child[rec_slot[(size_t)first_rec[t]]]; // the leaf, then its ancestors
        double a0 = 0.0, a2 = 0.0, b0, b2;
        bool any = false;
        while (skip_bounds(hs, e.n, e.p, child, b0, b2) && b0 < 1.0) {
            any = true, a0 = b0, a2 = b2;
            e.ref = device_child_word(child);
            if (at <= 0) break; // the root has no word
            child = at, at = parent[(size_t)at];
            if (at < 0) break;
        }
        if (!any) continue;
        const uint16_t h0 = half_up(a0), h2 = half_up(a2);
        if (h0 == 0x7C00 || h2 == 0x7C00) continue;
        e.a = (uint32_t)h0 | ((uint32_t)h2 << 16);
        hs.skip[t] = e;
    }
}


} // namespace rt
