// rt_bounce.h — one bounce of a path after its closest-hit query, as the render kernels (rt_kernels.h) and the path queries (rt_path_query.hip)
// run it: the ray's direction out of its half storage, shade_bounce and the Russian roulette. (Apart from rt_kernels.h, which defines the
// renderers' kernels and belongs to rt_frame.hip alone. rt_probe_kernels.h reads it for skip_entry, the origin skip's entry load.)
#pragma once
#include "rt_device.h"

namespace rt {

RT_DEV f3 ray_dir(const RayState& r) { return mk3(h2f(r.dir[0]), h2f(r.dir[1]), h2f(r.dir[2])); }

// the part of one bounce after the closest-hit query: unpack halves -> shade_hit -> repack (the body of
// render_pixel's loop, src/render_megakernel.cpp:34-55, and of shoot_rays, src/render_wavefront.cpp:245-291)
// FROM_TRAV (the kernels whose lanes keep a ray across shading rounds): origin and direction are READ from the traversal state — T.o
// and T.d are r.org and h2f(r.dir) exactly, trav_begin put them there — so that r.org / r.dir are written here and consumed by the
// trav_begin (or the queue store) that follows, live only inside the round: six lane registers less through the traversal loop.
// (with `tab`: the kernel's staged shading tables; without: the memory path only)
// `sink`: see shade_hit
template <bool FROM_TRAV = false, class Sink = NoSink>
RT_DEV bool shade_bounce(const SceneDev& S, uint32_t& rng, RayState& r, const Hit& h, f3& result, const Trav* T = nullptr, const ShadeTables* tab = nullptr,
                         long long* ck = nullptr, const Sink& sink = Sink{}) {
    f3 org = FROM_TRAV ? T->o : r.org;
    f3 dir = FROM_TRAV ? T->d : ray_dir(r);
    f3 att = mk3(h2f(r.att[0]), h2f(r.att[1]), h2f(r.att[2]));
    f3 rad = mk3(h2f(r.rad[0]), h2f(r.rad[1]), h2f(r.rad[2]));
    const bool done = FROM_TRAV ? shade_hit<true>(S, *tab, rng, h, org, dir, att, rad, result, ck, sink) : shade_hit<false>(S, ShadeTables{}, rng, h, org, dir, att, rad, result, nullptr, sink);
    r.org = org;
    r.dir[0] = f2h(dir.x), r.dir[1] = f2h(dir.y), r.dir[2] = f2h(dir.z);
    r.att[0] = f2h(att.x), r.att[1] = f2h(att.y), r.att[2] = f2h(att.z);
    r.rad[0] = f2h(rad.x), r.rad[1] = f2h(rad.y), r.rad[2] = f2h(rad.z);
    return done;
}

// The origin skip of the ray trav_begin has just started (rt_types.h: SkipRec, origin_skip_word): `tri` is the triangle the ray starts on, kNoTri
// for a camera ray or a ray out of a queue. The test runs on T.o and T.d, the origin and the direction (out of its half storage) that are
// traversed; the word goes to the lane's LDS slot above its stack, where trav_inner<true> reads it. One 32-byte entry per bounce ray, loaded
// by every lane (a lane without a triangle reads entry 0 and keeps kSkipNone): no exec-mask region of its own.
RT_DEV void origin_skip_none(const TravStack& stack) { *lds_at(skip_word_addr(stack)) = (int32_t)kSkipNone; }
// one entry out of memory: two 16-byte loads and their words (origin_skip below and k_probe_origin_skip, rt_probe_kernels.h, read it this way)
RT_DEV SkipRec skip_entry(const SkipRec* at) {
    const u32x4* ep = reinterpret_cast<const u32x4*>(at);
    const u32x4 a = ep[0], b = ep[1];
    SkipRec e;
    e.ref = a.x, e.n[0] = __uint_as_float(a.y), e.n[1] = __uint_as_float(a.z), e.n[2] = __uint_as_float(a.w);
    e.p[0] = __uint_as_float(b.x), e.p[1] = __uint_as_float(b.y), e.p[2] = __uint_as_float(b.z), e.a = b.w;
    return e;
}
RT_DEV void origin_skip(const SceneDev& S, uint32_t tri, const Trav& T, const TravStack& stack) {
    const SkipRec e = skip_entry(S.skip + (tri == kNoTri ? 0u : tri));
    const float o[3] = {T.o.x, T.o.y, T.o.z}, d[3] = {T.d.x, T.d.y, T.d.z};
    const uint32_t w = origin_skip_word(e, o, d);
    *lds_at(skip_word_addr(stack)) = (int32_t)(tri == kNoTri ? kSkipNone : w);
}

// Russian roulette on a continuing path (extension, see rt_renderer_set_russian_roulette); false = path ends
RT_DEV bool roulette(uint32_t& rng, RayState& r) {
    const float qx = h2f(r.att[0]), qy = h2f(r.att[1]), qz = h2f(r.att[2]);
    const float p = __builtin_fminf(__builtin_fmaxf(__builtin_fmaxf(qx, __builtin_fmaxf(qy, qz)), 0.05f), 1.0f);
    const float u = rng_next(rng);
    if (!(u < p)) return false;
    r.att[0] = f2h(qx / p), r.att[1] = f2h(qy / p), r.att[2] = f2h(qz / p);
    return true;
}

} // namespace rt
