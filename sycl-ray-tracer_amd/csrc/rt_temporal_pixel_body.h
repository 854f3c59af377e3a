// rt_temporal_pixel_body.h — what one thread of the temporal kernels does, as TEXT: included inside the body of k_temporal (rt_temporal.hip, with
// `constexpr bool MOMENTS = false`) and of k_temporal_moments (rt_temporal_moments.hip, MOMENTS = true), in the scope of their parameters
// (a, frame, nrm, pos, prv, h_col, h_pos, h_nrm, o_col, o_pos, o_nrm, out_f32, out_u8, hist_len; h_mom, o_mom, moments with MOMENTS).
// Why text and not a function template on the flag, as rt_gbuffer_pixel.h is: k_temporal must keep the instructions it had, and through an
// inlined function it does not. The by-value TemporalArgs then reaches its uses through a copy that is only resolved after inlining; the loads
// of the kernel arguments lose the compiler's not-clobbered marking and move, and about 900 lines of the listing change (registers, the order
// of scalar loads, branch structure). Passing the fields as scalars changes the listing too (their conditions fold differently). Included as
// text, the compiler sees for MOMENTS = false exactly the function it saw before.
// MOMENTS (rt_temporal_accumulate_moments): beside the colour, the moments M = (l, l*l) of the frame's luminance are blended with the history's,
// fetched through the same valid taps with the same weights; h_mom / o_mom are the previous and the current set's moment planes, `moments` the
// call's output (may be null: a plain rt_temporal_accumulate on an accumulator that has moments keeps them up to date).
// a 1-D grid of 64 x 4 tiles, row-major (as k_atrous)
const int32_t W = a.W, H = a.H;
const uint32_t tiles_x = ((uint32_t)W + 63u) / 64u;
const int32_t x = (int32_t)((blockIdx.x % tiles_x) * 64u + threadIdx.x), y = (int32_t)((blockIdx.x / tiles_x) * 4u + threadIdx.y);
if (x >= W || y >= H) return;
const int32_t p = y * W + x;
const float4 F = frame[p], N = nrm[p], P = pos[p];
const bool hit = __builtin_isfinite(P.w);
const float lx = F.x * F.x, ly = F.y * F.y, lz = F.z * F.z;
float ox = lx, oy = ly, oz = lz, n_new = hit ? 1.0f : 0.0f;
float m1 = 0.0f, m2 = 0.0f;
if constexpr (MOMENTS) {
    m1 = (lx * 0.2126f + ly * 0.7152f) + lz * 0.0722f;
    m2 = m1 * m1;
}
bool blended = false;
if (a.has_prev && hit) {
    const float4 Q = prv[p];
    const float rx = Q.x - a.c[0], ry = Q.y - a.c[1], rz = Q.z - a.c[2];
    const float s = a.em / dot3f(rx, ry, rz, a.m[0], a.m[1], a.m[2]);
    if (__builtin_isfinite(s) && s > 0.0f) {
        const float hx = rx * s - a.e[0], hy = ry * s - a.e[1], hz = rz * s - a.e[2];
        const float sx = dot3f(hx, hy, hz, a.du[0], a.du[1], a.du[2]) / a.dudu;
        const float sy = dot3f(hx, hy, hz, a.dv[0], a.dv[1], a.dv[2]) / a.dvdv;
        if (sx > -1.0f && sx < (float)W && sy > -1.0f && sy < (float)H) { // (NaN fails here, before any conversion to an integer)
            const float x0f = __builtin_floorf(sx), y0f = __builtin_floorf(sy);
            const float fx = sx - x0f, fy = sy - y0f;
            const float gx = 1.0f - fx, gy = 1.0f - fy;
            const int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;
            // The four taps' guides are fetched at once, from addresses clamped into the image (a tap outside it is dropped below): four
            // independent loads per plane in flight instead of a chain of dependent ones. The colour is read only where the guides passed.
            int32_t q[4];
            float w[4];
            bool valid[4];
            float4 Pt[4], Nt[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = k & 1, j = k >> 1; // tap order (0,0), (1,0), (0,1), (1,1)
                const int32_t tx = x0 + i, ty = y0 + j;
                w[k] = (i ? fx : gx) * (j ? fy : gy);
                valid[k] = tx >= 0 && tx < W && ty >= 0 && ty < H && w[k] > 0.0f;
                q[k] = min(max(ty, 0), H - 1) * W + min(max(tx, 0), W - 1);
                Pt[k] = h_pos[q[k]];
            }
            if (a.cos_normal != -1.0f) {
#pragma unroll
                for (int k = 0; k < 4; ++k) Nt[k] = h_nrm[q[k]];
            }
            float wsum = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, n_min = __builtin_inff();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bool ok = valid[k] && __builtin_isfinite(Pt[k].w); // (a miss of the previous frame: its stored length is 0)
                if (a.kx != 0.0f) {
                    const float dx = Pt[k].x - Q.x, dy = Pt[k].y - Q.y, dz = Pt[k].z - Q.z;
                    ok = ok && dot3f(dx, dy, dz, dx, dy, dz) * a.kx <= 1.0f;
                }
                if (a.cos_normal != -1.0f) ok = ok && dot3f(N.x, N.y, N.z, Nt[k].x, Nt[k].y, Nt[k].z) >= a.cos_normal;
                valid[k] = ok;
            }
            float4 Ct[4];
            float2 Mt[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (valid[k]) {
                    Ct[k] = h_col[q[k]];
                    if constexpr (MOMENTS) Mt[k] = h_mom[q[k]];
                }
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!valid[k]) continue;
                wsum = wsum + w[k];
                sr = sr + w[k] * Ct[k].x, sg = sg + w[k] * Ct[k].y, sb = sb + w[k] * Ct[k].z;
                n_min = __builtin_fminf(n_min, Ct[k].w);
                if constexpr (MOMENTS) s1 = s1 + w[k] * Mt[k].x, s2 = s2 + w[k] * Mt[k].y;
            }
            if (wsum >= kMinTapWeight) {
                const float n_next = __builtin_fminf(n_min + 1.0f, a.max_history);
                if (n_next != 1.0f) {
                    const float hr = sr / wsum, hg = sg / wsum, hb = sb / wsum;
                    const float alpha = 1.0f / n_next;
                    ox = hr + (lx - hr) * alpha, oy = hg + (ly - hg) * alpha, oz = hb + (lz - hb) * alpha;
                    n_new = n_next;
                    blended = true;
                    if constexpr (MOMENTS) {
                        const float h1 = s1 / wsum, h2 = s2 / wsum;
                        m1 = h1 + (m1 - h1) * alpha, m2 = h2 + (m2 - h2) * alpha;
                    }
                }
            }
        }
    }
}
o_col[p] = make_float4(ox, oy, oz, n_new);
o_pos[p] = P;
o_nrm[p] = N;
if constexpr (MOMENTS) {
    o_mom[p] = make_float2(m1, m2);
    if (moments) moments[p] = make_float2(m1, m2);
}
// without history the outputs are the input's own values, not the square root of their squares
const float fr = blended ? __builtin_sqrtf(ox) : F.x, fg = blended ? __builtin_sqrtf(oy) : F.y, fb = blended ? __builtin_sqrtf(oz) : F.z;
if (out_f32) out_f32[p] = make_float4(fr, fg, fb, 1.0f);
if (out_u8) out_u8[p] = make_uchar4(to_unorm8(fr), to_unorm8(fg), to_unorm8(fb), 255);
if (hist_len) hist_len[p] = n_new;
