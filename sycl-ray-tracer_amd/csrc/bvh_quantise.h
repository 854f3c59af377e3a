// bvh_quantise.h — the device's BVH4 node quantiser, shared by the device builder (lbvh_gpu.hip) and the device refit of dynamic scenes
// (rt_update.hip). It follows the host's rules (scene_build.cpp: quantise_node) and is pinned against them by tests/test_gpu_lbvh.py.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_types.h"

namespace rt {

struct Box3 {
    float lo[3], hi[3];
};

__device__ __forceinline__ float grid_step_dev(uint32_t biased_exp) { return __uint_as_float(biased_exp << 23); }

// quantises the padded boxes of the nk children of one node (same rules as the host's quantise_node). Returns false, like the host's,
// on a non-finite padded box or when no grid step up to 2^121 fits; every word is written all the same (an axis that did not fit keeps
// the empty pattern qlo 255, qhi 0), so a failed node holds nothing stale.
__device__ inline bool quantise_node_dev(BvhNode& n, int nk, const Box3* kb, float pad) {
    float nlo[3];
    n.scale_x = n.scale_y = n.scale_z = 1.0f;
    n.origin[0] = n.origin[1] = n.origin[2] = 0.0f;
    for (int i = 0; i < 6; ++i) n.q[i] = (i & 1) ? 0u : 0xFFFFFFFFu;
    for (int a = 0; a < 3; ++a) {
        float lo = kb[0].lo[a] - pad, hi = kb[0].hi[a] + pad;
        for (int k = 1; k < nk; ++k) lo = fminf(lo, kb[k].lo[a] - pad), hi = fmaxf(hi, kb[k].hi[a] + pad);
        nlo[a] = lo;
        n.origin[a] = lo;
        if (!isfinite(lo) || !isfinite(hi)) return false;
        const double ext = (double)hi - (double)lo;
        int e = ext > 0 ? (int)ceil(log2(ext / 255.0)) : -100;
        e = e < -100 ? -100 : (e > 100 ? 100 : e);
        for (;; ++e) {
            const float s = grid_step_dev((uint32_t)(e + 127));
            uint32_t lo_b = 0, hi_b = 0;
            bool ok = true;
            for (int k = 0; k < 4 && ok; ++k) {
                uint32_t ql = 255, qh = 0;
                if (k < nk) {
                    const float klo = kb[k].lo[a] - pad, khi = kb[k].hi[a] + pad;
                    const double fl = floor(((double)klo - (double)nlo[a]) / (double)s);
                    const double fh = ceil(((double)khi - (double)nlo[a]) / (double)s);
                    long il = (long)fmax(0.0, fmin(255.0, fl)), ih = (long)fmax(0.0, fmin(256.0, fh));
                    while (il > 0 && n.origin[a] + (float)il * s > klo) --il;
                    while (ih <= 255 && n.origin[a] + (float)ih * s < khi) ++ih;
                    if (ih > 255 || n.origin[a] + (float)il * s > klo) { ok = false; break; }
                    ql = (uint32_t)il, qh = (uint32_t)ih;
                }
                lo_b |= ql << (8 * k), hi_b |= qh << (8 * k);
            }
            if (ok) {
                n.q[2 * a] = lo_b, n.q[2 * a + 1] = hi_b;
                if (a == 0) n.scale_x = s;
                else if (a == 1) n.scale_y = s;
                else n.scale_z = s;
                break;
            }
            if (e > 120) return false;
        }
    }
    return true;
}

} // namespace rt
