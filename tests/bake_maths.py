"""Float64 references for the baked-lighting tables (the probe volume, the reflection probes, the lightmap), written from the mathematics
and from the published conventions of include/rt_mi355x.h (the SH order, the cube's face table, the texel-space triangle), not from the
header's fp32 arithmetic: tests/test_bake_maths.py holds the numpy models to them, tests/test_gpu_bake_maths.py the device.

The identity everything about the bakes hangs on: at max_depth = 1 a path is one ray, which returns the sky on a miss and (0, 0, 0) on a hit
of a surface that does not emit. So every bake output at depth 1 is sky x an integral of a binary visibility function over simple geometry,
and Gauss-Legendre quadrature in float64 gives that integral to machine precision. The scenes are rectangles on the faces of the unit cube
[-1, 1]^3 (patch_scene), seen from points inside it."""
import math

import numpy as np

from rtamd import scenes

f32, f64 = np.float32, np.float64
U = 2.0 ** -24  # the unit roundoff of fp32: half an ulp, relative


# ---- spherical harmonics and the cosine lobe ------------------------------------------------------------------------------------------------
def real_sh(d):
    """The nine real spherical harmonics of bands 0 to 2 at unit directions d (..., 3) -> (..., 9) float64, from their closed forms, in the
    published order: 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2 (the Condon-Shortley phase dropped: every band-1 term has a plus sign)."""
    d = np.asarray(d, f64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    pi = math.pi
    c0, c1 = 0.5 * math.sqrt(1.0 / pi), math.sqrt(3.0 / (4.0 * pi))
    c2, c20, c22 = 0.5 * math.sqrt(15.0 / pi), 0.25 * math.sqrt(5.0 / pi), 0.25 * math.sqrt(15.0 / pi)
    return np.stack([np.full(x.shape, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c20 * (3.0 * z * z - 1.0), c2 * x * z,
                     c22 * (x * x - y * y)], -1)


def _gauss_legendre(n, a, b):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w


def lobe_kernel(n, n_mu=12, n_phi=24):
    """K_k(n) = (1 / pi) * the integral over the hemisphere about n of Y_k(w) (n . w) dw, for normals n (m, 3) -> (m, 9) float64, by
    quadrature in a frame about n / |n|: Gauss-Legendre in mu = cos(theta) on [0, 1] and equispaced phi. Y_k (n . w) is a polynomial of
    degree 3 in w: the terms odd in sin(theta) vanish under any equispaced phi rule of more than 3 points, the others are polynomials of
    degree <= 3 in mu, so the rule is exact up to float64 rounding. The irradiance over pi of a table c is sum_k c_k K_k(n)."""
    assert n_mu >= 8 and n_phi >= 16
    n = np.asarray(n, f64).reshape(-1, 3)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    helper = np.where((np.abs(n[:, :1]) < 0.6), np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    t = np.cross(n, helper)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    mu, wmu = _gauss_legendre(n_mu, 0.0, 1.0)
    phi = (np.arange(n_phi) + 0.5) * (2.0 * math.pi / n_phi)
    MU, PHI = np.meshgrid(mu, phi, indexing="ij")
    WT = (wmu[:, None] * np.full(n_phi, 2.0 * math.pi / n_phi)[None, :]).reshape(-1)
    mu_, st = MU.reshape(-1), np.sqrt(1.0 - MU.reshape(-1) ** 2)
    cp, sp = np.cos(PHI.reshape(-1)), np.sin(PHI.reshape(-1))
    w = (st * cp)[None, :, None] * t[:, None, :] + (st * sp)[None, :, None] * b[:, None, :] + mu_[None, :, None] * n[:, None, :]  # (m, q, 3)
    return np.einsum("mqk,q->mk", real_sh(w), WT * mu_) / math.pi


def irradiance_over_pi(coef, n):
    """(1 / pi) * the integral over n . w > 0 of sum_k c_k Y_k(w) (n . w) dw for tables coef (m, 9, C) and normals n (m, 3) -> (m, C)"""
    return np.einsum("mkc,mk->mc", np.asarray(coef, f64), lobe_kernel(n))


def trilinear(origin, spacing, count, valid, pos):
    """The eight corners of the cell around each point pos (n, 3) of a count[0] x count[1] x count[2] grid (probe (iz * count[1] + iy) *
    count[0] + ix at origin + i * spacing) and their trilinear weights in float64 -> (index (n, 8) int64, weight (n, 8) float64). A point
    outside the grid is clamped onto it; the weights of invalid probes (valid (probes,) bool) are dropped and the others renormalised to sum
    1; where every corner is invalid all eight weights are 0."""
    origin, spacing, pos = np.asarray(origin, f64), np.asarray(spacing, f64), np.asarray(pos, f64)
    n = len(pos)
    idx, wts = np.zeros((n, 8), np.int64), np.ones((n, 8))
    cell = []
    for a in range(3):
        g = np.clip((pos[:, a] - origin[a]) / spacing[a], 0.0, count[a] - 1.0)
        i0 = np.minimum(np.floor(g).astype(np.int64), max(count[a] - 2, 0))
        cell.append((i0, g - i0))
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        i = [np.minimum(cell[a][0] + d, count[a] - 1) for a, d in enumerate((dx, dy, dz))]
        idx[:, c] = (i[2] * count[1] + i[1]) * count[0] + i[0]
        for a, d in enumerate((dx, dy, dz)):
            wts[:, c] *= cell[a][1] if d else 1.0 - cell[a][1]  # (the upper corner of an axis with one probe has f = 0: weight 0)
    wts = np.where(np.asarray(valid, bool)[idx], wts, 0.0)
    W = wts.sum(1, keepdims=True)
    return idx, np.where(W > 0, wts / np.where(W > 0, W, 1.0), 0.0)


# ---- the unit cube: the header's face table, its world <-> face map written out by hand ---------------------------------------------------
def face_point(f, s, t):
    """The world point (= unnormalised direction from the origin) of face f at face coordinates (s, t): the table of include/rt_mi355x.h"""
    s, t = np.asarray(s, f64), np.asarray(t, f64)
    one = np.ones_like(s)
    return np.stack({0: (one, -t, -s), 1: (-one, -t, s), 2: (s, one, t), 3: (s, -one, -t), 4: (s, -t, one), 5: (-s, -t, -one)}[int(f)], -1)


def face_coords(f, p):
    """The inverse on face f's plane: world points p (..., 3) -> (s, t, h), h the coordinate along the face's outward axis"""
    p = np.asarray(p, f64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return {0: (-z, -y, x), 1: (z, -y, -x), 2: (x, z, y), 3: (x, -z, -y), 4: (x, -y, z), 5: (-x, -y, -z)}[int(f)]


def cube_hit(eye, d):
    """Where rays from eye (3,), a point inside the unit cube, along d (n, 3) leave the cube -> (face (n,), s (n,), t (n,)) in float64"""
    eye, d = np.asarray(eye, f64), np.asarray(d, f64)
    with np.errstate(all="ignore"):
        ta = np.where(d != 0, (np.sign(d) - eye[None, :]) / d, np.inf)
    axis = np.argmin(ta, 1)
    p = eye[None, :] + d * ta[np.arange(len(d)), axis][:, None]
    face = 2 * axis + (d[np.arange(len(d)), axis] < 0)
    s, t = np.zeros(len(d)), np.zeros(len(d))
    for f in range(6):
        m = face == f
        s[m], t[m] = face_coords(f, p[m])[:2]
    return face, s, t


def rect_integrals(face_rect, funcs, eye=(0.0, 0.0, 0.0), n=48):
    """The integrals of funcs over the solid angle that the rectangle face_rect = (face, s0, s1, t0, t1) on a face plane of the unit cube
    subtends at `eye` (a point on the inner side of that plane) -> one array per func. Seen from the eye the rectangle is the rectangle
    [(s0 - es) / h, (s1 - es) / h] x [..t..] on a plane at distance 1, (es, et) the eye's face coordinates and h its distance to the plane;
    there d(omega) = ds dt / (1 + s^2 + t^2)^(3/2), and Gauss-Legendre in (s, t) with n x n points converges to float64 rounding for these
    smooth integrands. Each func maps unit world directions (m, 3) to (m, ...) values."""
    assert n >= 32
    f, s0, s1, t0, t1 = face_rect
    es, et, eh = face_coords(f, np.asarray(eye, f64))
    h = 1.0 - eh
    assert h > 0
    s, ws = _gauss_legendre(n, (s0 - es) / h, (s1 - es) / h)
    t, wt = _gauss_legendre(n, (t0 - et) / h, (t1 - et) / h)
    S, T = (a.reshape(-1) for a in np.meshgrid(s, t, indexing="ij"))
    w = (ws[:, None] * wt[None, :]).reshape(-1) / (1.0 + S * S + T * T) ** 1.5
    d = face_point(f, S, T)  # a direction in world axes: the face frame is the same whatever the eye
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return [np.tensordot(w, np.asarray(fn(d), f64), axes=(0, 0)) for fn in funcs]


def sh_moments(rects, eye=(0.0, 0.0, 0.0)):
    """For a probe at `eye` among rectangles that block the sky: (F (9,), G (9,)) = the sums over the rectangles of the integrals of Y_k
    and of Y_k^2 over their solid angles"""
    F, G = np.zeros(9), np.zeros(9)
    for r in rects:
        a, b = rect_integrals(r, [real_sh, lambda d: real_sh(d) ** 2], eye)
        F, G = F + a, G + b
    return F, G


def sh_expectation(rects, dirs, eye=(0.0, 0.0, 0.0)):
    """What a depth-1 bake of `dirs` uniform directions estimates at `eye`, per unit of sky -> (mean (9,), sigma (9,), magnitude (9,)):
    mean_k = sqrt(4 pi) delta_k0 - F_k, sigma_k = 4 pi sqrt(Var[V Y_k] / dirs) the estimator's standard deviation (V the visibility of a
    uniform direction), magnitude_k = 4 pi sqrt(E[(V Y_k)^2]) >= 4 pi E|V Y_k|, a bound on the sum of the estimator's term magnitudes."""
    F, G = sh_moments(rects, eye)
    four_pi = 4.0 * math.pi
    mean = -F
    mean[0] += math.sqrt(four_pi)
    e1, e2 = mean / four_pi, (1.0 - G) / four_pi  # the integral of Y_k^2 over the sphere is 1
    return mean, four_pi * np.sqrt(np.maximum(e2 - e1 * e1, 0.0) / dirs), four_pi * np.sqrt(e2)


def patch_scene(rects, name="patches"):
    """One quad per face rectangle (face, s0, s1, t0, t1) on the planes of the unit cube, one diffuse material, the default sky"""
    b = scenes.SceneBuilder(name)
    mat = b.add_material(scenes.Material(color=(0.7, 0.6, 0.5)))
    for f, s0, s1, t0, t1 in rects:
        c = face_point(f, np.array([s0, s1, s1, s0]), np.array([t0, t0, t1, t1]))
        b.add_instance(b.add_mesh(*scenes.mesh_quad(c[0], c[1], c[2], c[3])), mat)
    return b.build()


def coverage(size, rect):
    """(size, size) float64 [y, x]: the fraction of each level-0 texel's (s, t) square inside rect = (face, s0, s1, t0, t1). Exact for a
    probe at the origin: the jitter is uniform in (s, t) and the rectangle lies on the face plane."""
    _, s0, s1, t0, t1 = rect
    edges = np.arange(size + 1) * (2.0 / size) - 1.0

    def overlap(a, b):
        return np.clip(np.minimum(edges[1:], b) - np.maximum(edges[:-1], a), 0.0, None) / (2.0 / size)
    return overlap(t0, t1)[:, None] * overlap(s0, s1)[None, :]


def texel_classes(size, rects, eye, margin=0.01):
    """For a capture at `eye`, a point inside the cube that need not be its centre: which level-0 texels see only a rectangle and which see
    none -> (open (6, size, size) bool, blocked (6, size, size) bool); a texel in neither is left unclassified. The four corners of a texel's
    (s, t) square are followed from the eye to the cube. A texel is blocked when all four land on one face inside its rectangle shrunk by
    `margin` (the rectangle is convex, and so is the texel's image on that plane). It is open when all four land on one face and their
    bounding box grown by `margin` misses that face's rectangle."""
    by_face = {r[0]: r for r in rects}
    edges = np.arange(size + 1) * (2.0 / size) - 1.0
    T, S = (a.reshape(-1) for a in np.meshgrid(edges, edges, indexing="ij"))
    is_open, blocked = np.zeros((6, size, size), bool), np.zeros((6, size, size), bool)
    for f in range(6):
        face, s, t = (a.reshape(size + 1, size + 1) for a in cube_hit(eye, face_point(f, S, T)))
        quad = lambda a: np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]])  # noqa: E731  (4, size, size) [corner, y, x]
        qf, qs, qt = quad(face), quad(s), quad(t)
        same = (qf == qf[0]).all(0)
        for g in range(6):
            on = same & (qf[0] == g)
            if g not in by_face:
                is_open[f] |= on
                continue
            _, s0, s1, t0, t1 = by_face[g]
            blocked[f] |= on & ((qs >= s0 + margin) & (qs <= s1 - margin) & (qt >= t0 + margin) & (qt <= t1 - margin)).all(0)
            is_open[f] |= on & ((qs.max(0) + margin < s0) | (qs.min(0) - margin > s1) | (qt.max(0) + margin < t0) | (qt.min(0) - margin > t1))
    return is_open, blocked


def binomial_interval(n, p_lo, p_hi, tail=5e-7):
    """(lo, hi): the counts k of Binomial(n, p) that are not in a tail of less than `tail` for some p in [p_lo, p_hi]"""
    def pmf(p):
        return [math.comb(n, k) * p ** k * (1.0 - p) ** (n - k) for k in range(n + 1)]
    low, high = pmf(min(max(p_lo, 0.0), 1.0)), pmf(min(max(p_hi, 0.0), 1.0))
    lo = 0
    while sum(low[:lo + 1]) < tail:
        lo += 1
    hi = n
    while sum(high[hi:]) < tail:
        hi -= 1
    return lo, hi


# ---- the lightmap: texel centres on their owners in float64 -------------------------------------------------------------------------------
def _texel_space(uv, W, H):
    """The triangles as the contract defines them in texel space: P_k = (u_k * (float)W, v_k * (float)H), one fp32 product each, widened
    -> (P (T, 3, 2) float64, ok (T,): six finite coordinates)"""
    with np.errstate(all="ignore"):
        P = (np.asarray(uv, f32).reshape(-1, 3, 2) * np.array([W, H], f32)).astype(f64)
    return P, np.isfinite(P).all(axis=(1, 2))


_FMAX = float(np.finfo(f32).max)


def _edge(A, B, qx, qy):
    """E(A, B, q) = (B.x - A.x) (q.y - A.y) - (B.y - A.y) (q.x - A.x) in float64 -> (value, the sum of its two products' magnitudes, exact:
    whether fp32 computes every one of its five operations without a rounding, nan: whether both products leave the fp32 range with one
    sign, where the contract's fp32 value is inf - inf, a NaN that covers nothing; one product beyond the range gives an infinity of the
    float64 value's sign)"""
    d1, d2, d3, d4 = B[..., 0] - A[..., 0], qy - A[..., 1], B[..., 1] - A[..., 1], qx - A[..., 0]
    p1, p2 = d1 * d2, d3 * d4
    e = p1 - p2
    exact = np.ones(np.broadcast(p1, p2).shape, bool)
    with np.errstate(all="ignore"):
        for v in (d1, d2, d3, d4, p1, p2, e):
            exact = exact & (v.astype(f32).astype(f64) == v)
    nan = (np.abs(p1) > _FMAX) & (np.abs(p2) > _FMAX) & (np.sign(p1) == np.sign(p2))
    return e, np.abs(p1) + np.abs(p2), exact, nan


def lightmap_ownership(uv, W, H, margin=4.0 * U):
    """Which triangle owns each texel of a W x H atlas, decided in float64 -> (owner (W * H,) int64, -1: none, sure (W * H,) bool). A centre
    is inside a triangle when its three edge values have the area's sign or are 0. An fp32 edge value differs from the float64 one by at
    most margin * (the sum of its products' magnitudes): the roundings of two differences and a product on either side at half an ulp each
    and one of the subtraction, under 4 * 2^-24. A texel is `sure` when, for every triangle, the centre is beyond that margin outside some
    edge, or every edge value is either further from 0 than the margin or computed without any rounding in fp32 (then the comparison with 0
    is the exact one). The owner of a sure texel is the lowest index whose triangle holds the centre."""
    P, ok = _texel_space(uv, W, H)
    owner, sure = np.full(W * H, -1, np.int64), np.ones(W * H, bool)
    cx, cy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5, indexing="xy")
    cx, cy = cx.reshape(-1), cy.reshape(-1)
    for t in np.flatnonzero(ok)[::-1]:  # the lowest index last: it takes the texel
        A, B, C_ = P[t, 0], P[t, 1], P[t, 2]
        area, _, _, area_nan = _edge(A, B, C_[0], C_[1])
        if area == 0 or area_nan:
            continue
        lo, hi = np.floor(P[t].min(0) - 1.5), np.ceil(P[t].max(0) + 1.5)
        box = np.flatnonzero((cx >= lo[0]) & (cx <= hi[0]) & (cy >= lo[1]) & (cy <= hi[1]))
        if len(box) == 0:
            continue
        inside, near, clearly_out = np.ones(len(box), bool), np.zeros(len(box), bool), np.zeros(len(box), bool)
        for a, b in ((B, C_), (C_, A), (A, B)):
            e, mag, exact, nan = _edge(a, b, cx[box], cy[box])
            e = e * np.sign(area)
            clear = exact | (np.abs(e) > margin * mag)
            inside &= (e >= 0) & ~nan
            near |= ~clear & ~nan
            clearly_out |= nan | ((e < 0) & clear)
        sure[box[near & ~clearly_out]] = False
        owner[box[inside]] = t
    return owner, sure


def texel_points(sd, uv, W, H, owner):
    """For the covered texels of owner (W * H,) (anything else than 0xFFFFFFFF / -1 is a triangle index): float64 barycentrics of the texel
    centre in its owner's texel-space triangle, the world point from SceneDesc.world_triangles(), and the normal: the interpolated vertex
    normal through a float64 inverse-transpose of the instance matrix, normalised. -> {"index": the covered texels, "pos", "normal": (n, 3)
    float64, "cond": (n,) the sum of the product magnitudes of the two edge functions used over |area|, "scale": (n,) the largest sum of
    term magnitudes in the world transform of the owner's corners, "edges": (n, 3) the three edge values with the area's sign, "mags":
    (n, 3) their product magnitudes, "blend": (n,) the length of the interpolated normal before it is normalised}"""
    owner = np.asarray(owner).astype(np.int64).reshape(-1)
    i = np.flatnonzero((owner >= 0) & (owner != 0xFFFFFFFF))
    t = owner[i]
    P, _ = _texel_space(uv, W, H)
    qx, qy = (i % W) + 0.5, (i // W) + 0.5
    A, B, C_ = P[t, 0], P[t, 1], P[t, 2]
    area = _edge(A, B, C_[:, 0], C_[:, 1])[0]
    (e0, m0), (e1, m1), (e2, m2) = (_edge(a, b, qx, qy)[:2] for a, b in ((B, C_), (C_, A), (A, B)))
    bx, by = e1 / area, e2 / area
    w = 1.0 - bx - by
    V = sd.world_triangles()[t]
    pos = w[:, None] * V[:, 0] + bx[:, None] * V[:, 1] + by[:, None] * V[:, 2]
    idx = np.asarray(sd.indices, np.int64).reshape(-1, 3)[t]
    n = np.asarray(sd.normals, f64)[idx]
    v = w[:, None] * n[:, 0] + bx[:, None] * n[:, 1] + by[:, None] * n[:, 2]
    inst = np.asarray(sd.tri_instance, np.int64)[t]
    M = np.asarray(sd.transforms, f64).reshape(-1, 4, 4).transpose(0, 2, 1)  # (column-major in the description)
    NM = np.linalg.inv(M[:, :3, :3]).transpose(0, 2, 1)
    g = np.einsum("nij,nj->ni", NM[inst], v)
    nrm = g / np.linalg.norm(g, axis=1, keepdims=True)
    obj = np.abs(np.asarray(sd.positions, f64)[idx])                                                 # (n, 3 corners, 3)
    terms = np.einsum("nij,ncj->nci", np.abs(M[inst][:, :3, :3]), obj) + np.abs(M[inst][:, None, :3, 3])
    sgn = np.sign(area)[:, None]
    return {"index": i, "pos": pos, "normal": nrm, "cond": (m1 + m2) / np.abs(area), "scale": terms.max(axis=(1, 2)),
            "edges": np.stack([e0, e1, e2], 1) * sgn, "mags": np.stack([m0, m1, m2], 1), "blend": np.linalg.norm(v, axis=1)}


# ---- the checks, shared by the numpy models' tests and the device's -----------------------------------------------------------------------
NONE = 0xFFFFFFFF
RATIOS = {}  # check -> the worst observed ratio of an error to its bound in this process (printed by the tests; DESIGN.md §2 keeps a table)


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))
    print(f"bake_maths: {what}: worst error / bound = {float(ratio):.3f}")


# The bound of the SH sample, in units of 2^-24 * M, M the sum of the term magnitudes w |K_k| |c_k|. First-order count of the fp32 roundings
# on one term's way through step 6: per axis the subtraction, the division and 1 - f (9); the two products of the corner weight (2); w * coef
# (1); S / W (1); B * C (1); up to four operations in Y_k(n) (4); the product with Y_k (1): 19. A term that enters an n-term running sum at
# place j passes n - j additions: on average 3.5 of the 7 over the corners and 4 of the 8 over k (7.5), and W passes its own 3.5. The two
# decimal constants that a term meets (B_k and the constant of Y_k) are off by up to half an ulp each (2). 19 + 7.5 + 3.5 + 2 = 32. The
# roundings of the corner weights enter S and W alike and are not counted twice.
SH_SAMPLE_ROUNDINGS = 9 + 2 + 1 + 1 + 1 + 4 + 1 + 7.5 + 3.5 + 2
assert SH_SAMPLE_ROUNDINGS == 32


def check_sh_sample(got, origin, spacing, count, sh, pos, nrm, what="sh sample"):
    """Step 6 of the probe volume against (1 / pi) * the cosine-weighted integral of the trilinearly interpolated radiance"""
    got, sh = np.asarray(got, f64), np.asarray(sh, f64).reshape(-1, 9, 4)
    idx, w = trilinear(origin, spacing, count, sh[:, 0, 3] != 0, pos)
    K = lobe_kernel(nrm)
    c = sh[idx][..., :3]                                           # (n, 8, 9, 3)
    ref = np.einsum("nc,nckj,nk->nj", w, c, K)
    M = np.einsum("nc,nckj,nk->nj", w, np.abs(c), np.abs(K))
    bound = SH_SAMPLE_ROUNDINGS * U * M
    assert got.shape == ref.shape and np.isfinite(got).all() and (got >= 0).all()
    dark = ref < -bound
    assert (got[dark] == 0).all(), f"{what}: {np.count_nonzero(got[dark])} outputs above 0 where the irradiance is negative"
    err = np.abs(got - ref)[~dark]
    bad = err > bound[~dark]
    with np.errstate(all="ignore"):
        ratio = np.where(bound[~dark] > 0, err / bound[~dark], np.where(err > 0, np.inf, 0.0))
    _note(what, ratio.max() if ratio.size else 0.0)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} outputs beyond 32 * 2^-24 * M, the worst at {ratio.max():.1f} bounds"
    return ref, dark


def check_sh_bake(sh, stats, rects, eyes, valid, dirs, sky, what="sh bake"):
    """A depth-1 bake of probes at `eyes` (probes, 3) among rectangles that block the sky: sky * (sqrt(4 pi) delta_k0 - sum F_k) within
    5 sigma_k + dirs * 2^-24 * (the terms' magnitudes); an invalid probe is zeros; rays = dirs per valid probe"""
    sh, sky = np.asarray(sh), np.asarray(sky, f64)
    worst = 0.0
    for p, eye in enumerate(np.asarray(eyes, f64)):
        if not valid[p]:
            assert (sh[p].view(np.uint32) == 0).all(), f"{what}: invalid probe {p} is not zeros"
            continue
        mean, sigma, mag = sh_expectation(rects, dirs, eye)
        tol = (5.0 * sigma + dirs * U * mag)[:, None] * sky[None, :]
        err = np.abs(sh[p, :, :3].astype(f64) - mean[:, None] * sky[None, :])
        worst = max(worst, (err / tol).max())
        assert (err <= tol).all(), f"{what}: probe {p}: error / tolerance per coefficient and channel\n{err / tol}"
        assert sh[p, 0, 3] == 1 and (sh[p, 1:, 3] == 0).all()
    _note(what, worst)
    n_valid = int(np.count_nonzero(valid))
    assert stats == {"probes": len(eyes), "valid": n_valid, "rays": dirs * n_valid}, stats


def check_cube_level0(level0, rects, spt, sky, what="cube level 0"):
    """Level 0 (6, S, S, 4) of a depth-1 capture at the origin among rectangles on the cube's faces: open texels are the sky, blocked ones 0,
    and a partly covered one holds a number of clear rays that Binomial(spt, 1 - coverage) allows"""
    level0, sky = np.asarray(level0), np.asarray(sky, f64)
    S = level0.shape[1]
    assert level0.shape == (6, S, S, 4) and (level0[..., 3] == 1).all()
    by_face = {r[0]: r for r in rects}
    widen = 2.0 ** -9 / (2.0 / S)
    worst, n_open, n_blocked, n_partial = 0.0, 0, 0, 0
    for f in range(6):
        cov = coverage(S, by_face[f]) if f in by_face else np.zeros((S, S))
        rgb = level0[f, :, :, :3].astype(f64)
        is_open, blocked = cov == 0, cov == 1
        err = np.abs(rgb[is_open] - sky) / (spt * U * sky)
        worst = max(worst, err.max())
        assert (err <= 1).all(), f"{what}: face {f}: {(err > 1).any(1).sum()} open texels are not the sky"
        assert (rgb[blocked] == 0).all(), f"{what}: face {f}: {(rgb[blocked] != 0).any(1).sum()} blocked texels are not 0"
        for y, x in zip(*np.nonzero(~is_open & ~blocked)):
            clear = rgb[y, x] / sky * spt
            c = int(round(clear[0]))
            assert (np.abs(clear - c) <= spt * U * spt).all(), f"{what}: face {f} texel ({x}, {y}): {clear} clear rays"
            lo, hi = binomial_interval(spt, 1.0 - cov[y, x] - widen, 1.0 - cov[y, x] + widen)
            assert lo <= c <= hi, f"{what}: face {f} texel ({x}, {y}): {c} of {spt} rays clear at coverage {cov[y, x]:.3f}, expected {lo} .. {hi}"
        n_open, n_blocked, n_partial = n_open + is_open.sum(), n_blocked + blocked.sum(), n_partial + (~is_open & ~blocked).sum()
    _note(what, worst)
    return int(n_open), int(n_blocked), int(n_partial)


def cube_sample_cases(S, rects, per_face=6):
    """World directions (float64, of several lengths) from the origin to the centres of level-0 texels whose in-face neighbours within two
    texels are all open or all blocked -> (dirs (n, 3), blocked (n,) bool)"""
    by_face = {r[0]: r for r in rects}
    c = (np.arange(S) + 0.5) * (2.0 / S) - 1.0
    dirs, blocked = [], []
    for f in range(6):
        cov = coverage(S, by_face[f]) if f in by_face else np.zeros((S, S))
        pad = np.pad(cov, 2, mode="edge")
        win = np.stack([pad[dy:dy + S, dx:dx + S] for dy in range(5) for dx in range(5)])
        for cls in (0.0, 1.0):
            ys, xs = np.nonzero((win == cls).all(0))
            pick = np.linspace(0, len(ys) - 1, min(per_face, len(ys))).astype(int) if len(ys) else []
            for k, j in enumerate(pick):
                dirs.append(face_point(f, c[xs[j]], c[ys[j]]) * (0.25 + 1.75 * k))
                blocked.append(cls == 1.0)
    return np.array(dirs), np.array(blocked)


def check_cube_classes(level0, is_open, blocked, spt, sky, what="cube level 0, off centre"):
    """Level 0 (6, S, S, 4) of a depth-1 capture against texel_classes: open texels are the sky, blocked ones 0, the others between"""
    level0, sky = np.asarray(level0), np.asarray(sky, f64)
    rgb = level0[..., :3].astype(f64)
    assert (level0[..., 3] == 1).all() and is_open.sum() > is_open.size // 4 and blocked.sum() >= 6 * 4 and not (is_open & blocked).any()
    err = np.abs(rgb[is_open] - sky) / (spt * U * sky)
    _note(what, err.max())
    assert (err <= 1).all(), f"{what}: {(err > 1).any(1).sum()} open texels are not the sky"
    assert (rgb[blocked] == 0).all(), f"{what}: {(rgb[blocked] != 0).any(1).sum()} blocked texels are not 0"
    assert (rgb >= 0).all() and (rgb <= sky * (1.0 + spt * U)).all()


def check_cube_samples(out, blocked, spt, sky, what="cube sample"):
    out, sky = np.asarray(out, f64), np.asarray(sky, f64)
    assert blocked.any() and (~blocked).any()
    assert (out[blocked] == 0).all(), f"{what}: {np.count_nonzero(out[blocked].any(1))} lookups of blocked texels are not 0"
    err = np.abs(out[~blocked] - sky) / (spt * U * sky)
    _note(what, err.max())
    assert (err <= 1).all(), f"{what}: {(err > 1).any(1).sum()} lookups of open texels are not the sky"


def check_lightmap(tri, pos, nrm, sd, uv, W, H, what="lightmap"):
    """Steps 1 and 2 of the lightmap against float64 geometry: the owner plane against lightmap_ownership, the points and normals against
    texel_points. The position bound is 8 * 2^-24 * scale * (1 + cond), the normal's 16 * 2^-24 (Euclidean) and 4 * 2^-23 off unit length."""
    tri = np.asarray(tri).reshape(-1).astype(np.int64)
    pos, nrm = np.asarray(pos, f64).reshape(-1, 3), np.asarray(nrm, f64).reshape(-1, 3)
    covered = tri != NONE
    assert covered.any()
    tp = texel_points(sd, uv, W, H, np.where(covered, tri, -1))
    i = tp["index"]
    bound = 8.0 * U * tp["scale"] * (1.0 + tp["cond"])
    err = np.abs(pos[i] - tp["pos"]).max(1)
    _note(f"{what}: position", (err / bound).max())
    assert (err <= bound).all(), f"{what}: {(err > bound).sum()} positions off their surface point, the worst at {(err / bound).max():.1f} bounds"
    nerr = np.linalg.norm(nrm[i] - tp["normal"], axis=1) / (16.0 * U)
    _note(f"{what}: normal", nerr.max())
    assert (nerr <= 1).all(), f"{what}: {(nerr > 1).sum()} normals off, the worst at {nerr.max():.1f} bounds (blend length {tp['blend'][nerr.argmax()]:.3f})"
    assert (np.abs(np.linalg.norm(nrm[i], axis=1) - 1.0) <= 4 * 2.0 ** -23).all()
    assert (tp["edges"] >= -4.0 * U * tp["mags"]).all(), f"{what}: a covered texel's centre lies outside its owner"
    owner, sure = lightmap_ownership(uv, W, H)
    share = np.count_nonzero(covered & ~sure) / np.count_nonzero(covered)
    print(f"bake_maths: {what}: {share:.4%} of the covered texels are within the margin of an edge")
    assert share <= 0.01, f"{what}: {share:.2%} of the covered texels are too close to an edge to call"
    want = np.where(owner < 0, NONE, owner)
    wrong = sure & (tri != want)
    assert not wrong.any(), f"{what}: {wrong.sum()} texels clear of every edge have another owner, the first at {np.flatnonzero(wrong)[:5]}"
    return share
