// bvh_quantise.h — the BVH4 node quantiser: one text for the host builders and the host refit (scene_build.cpp), the device builder
// (lbvh_gpu.hip) and the device refit of dynamic scenes (rt_update.hip). tests/test_gpu_lbvh.py holds the device's results against the
// host's: what could still differ between them is the two math libraries (log2, ceil), not the rules.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <math.h>

#include "rt_types.h"

namespace rt {

RT_HD float grid_step(uint32_t biased_exp) { return __builtin_bit_cast(float, biased_exp << 23); } // 2^(e-127), exactly as the kernels decode it

// Quantises the boxes of the nk children of one node, each padded by `pad` first. Returns false on a non-finite padded box or when no grid
// step up to 2^121 fits; every word is written all the same (an axis that did not fit keeps the empty pattern), so a failed node holds
// nothing stale.
RT_HD bool quantise_node(BvhNode& n, int nk, const Box3* kb, float pad) {
    float nlo[3];
    clear_planes(n);
    for (int a = 0; a < 3; ++a) {
        float lo = kb[0].lo[a] - pad, hi = kb[0].hi[a] + pad;
        for (int k = 1; k < nk; ++k) lo = fminf(lo, kb[k].lo[a] - pad), hi = fmaxf(hi, kb[k].hi[a] + pad);
        nlo[a] = lo;
        n.origin[a] = lo;
        if (!isfinite(lo) || !isfinite(hi)) return false;
        const double ext = (double)hi - (double)lo;
        int e = ext > 0 ? (int)ceil(log2(ext / 255.0)) : -100;
        e = e < -100 ? -100 : (e > 100 ? 100 : e);
        for (;; ++e) { // raise the grid step until every plane fits in 8 bits
            const float s = grid_step((uint32_t)(e + 127));
            uint32_t lo_b = 0, hi_b = 0;
            bool ok = true;
            for (int k = 0; k < 4 && ok; ++k) {
                uint32_t ql = 255, qh = 0; // absent child: the inverted box
                if (k < nk) {
                    const float klo = kb[k].lo[a] - pad, khi = kb[k].hi[a] + pad;
                    const double fl = floor(((double)klo - (double)nlo[a]) / (double)s);
                    const double fh = ceil(((double)khi - (double)nlo[a]) / (double)s);
                    long il = (long)fmax(0.0, fmin(255.0, fl)), ih = (long)fmax(0.0, fmin(256.0, fh));
                    // verify with the kernel's own float decode; nudge outwards if rounding bit us
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
