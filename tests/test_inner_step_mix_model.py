"""The arithmetic of the mixed-precision plane decode that EXPERIMENTS.md ("The inner step: mixed fmas") measured and did not keep, in exact
rational arithmetic with ONE rounding to fp32 per fma — the model scripts/valu_calib_mix.hip's device check stands on.

The inner step computes every plane distance as t = fma((float)q, a, b): q a byte of the node, a = scale * (1 / d), b = origin * (1 / d) - o * (1 / d).
  denormal form   v_perm_b32 makes two bytes of a plane word two halves with a zero high byte, {0, b1, 0, b0} and {0, b3, 0, b2}: the fp16
                  denormals q * 2^-24. v_fma_mix_f32 widens a half exactly and rounds half * a24 + b once, a24 = a * 2^24 (v_ldexp_f32, exact):
                  (q * 2^-24) * (a * 2^24) = q * a, so t is fma((float)q, a, b) bit for bit — as long as a24 is finite.
  a24 overflows   a node's scale is a power of two up to 2^20 (bvh_quantise.h: extent < 2e8 + padding, 255 steps) and trav_begin clamps |d| to
                  1e-30: a = 2^20 * 1e30 is finite, a24 is not, and 0 * inf = NaN loses the child with q = 0. 2^-83 is the smallest power of
                  two as a clamp that keeps a24 finite (2^127).
  fallback form   high byte 0x3C (selector byte 4 .. 7 picks a byte of the first source, the integer 60): the half 1 + q / 1024, a normal
                  number. a' = a * 2^10 (exact), b' = fl(b - a'), t' = fl(half * a' + b') = fl(q * a + a' + b'). Against t = fl(q * a + b) the one
                  new error is b' - (b - a'), at most half an ulp of b - a'; with the two final roundings
                      |t' - t| <= 2^-24 * (|b - a'| + |t| + |t'|)      (ulp(x) / 2 <= 2^-24 |x| for normal x)
                  which is "about |a'| * 2^-24" where a' dominates b — 1 / 16384 of a grid step. Not bit for bit: it was not built."""
from fractions import Fraction

import numpy as np

f32 = np.float32
K_PERM_LO, K_PERM_HI = 0x0C010C00, 0x0C030C02
OLD_CLAMP, MIX_CLAMP = float(f32(1e-30)), 2.0 ** -83
MAX_SCALE = 2.0 ** 20  # ceil(log2((2e8 + padding) / 255)) = 20
INF = Fraction(2) ** 128


def fl(x):
    """one rounding of an exact rational to fp32, nearest-even, denormals kept; None for an overflow (the fma's +-inf)"""
    if x == 0:
        return Fraction(0)
    s, m = (-1 if x < 0 else 1), abs(x)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    assert Fraction(2) ** e <= m < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = m / quantum
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k & 1):
        k += 1
    r = k * quantum
    return None if r >= INF else s * r


def half_value(h):
    s, e, m = h >> 15, (h >> 10) & 31, h & 1023
    assert e != 31
    v = Fraction(m, 1 << 24) if e == 0 else Fraction(1024 + m) * Fraction(2) ** (e - 25)
    return -v if s else v


def perm(s0, s1, selector):
    """v_perm_b32: result byte i = byte selector_i of {s0, s1} (0 .. 3: s1, 4 .. 7: s0), 0x0C: 0x00"""
    both = (s0 << 32) | s1
    out = 0
    for i in range(4):
        k = (selector >> (8 * i)) & 0xFF
        assert k < 8 or k == 0x0C
        out |= (0 if k == 0x0C else (both >> (8 * k)) & 0xFF) << (8 * i)
    return out


def mix(h16, a, b):
    """v_fma_mix_f32 with a half first operand"""
    return fl(half_value(h16) * a + b)


def sample(n=96):
    """(a, b) as the step meets them: a = scale / d, b up to 1e8 / d; negative, tiny (denormal a) and clamped-direction values among them"""
    rng = np.random.default_rng(20)
    out = []
    for i in range(n):
        scale = 2.0 ** int(rng.integers(-100, 21))
        kind = i % 4
        if kind == 0:
            d = MIX_CLAMP  # a direction component that is zero
        elif kind == 1:
            d = float(f32(2.0 ** -24 * rng.integers(1, 1024)))  # the smallest halves
        else:
            d = float(f32(rng.uniform(1e-3, 1.0)))
        d *= float(rng.choice([-1.0, 1.0]))
        inv = f32(1.0) / f32(d)
        a = f32(scale) * inv
        b = f32(rng.uniform(-1e8, 1e8)) * inv if kind != 3 else f32(rng.uniform(-1.0, 1.0) * 2.0 ** int(rng.integers(-140, 0)))
        if i % 16 == 15:
            a = f32(rng.choice([-1.0, 1.0]) * 2.0 ** int(rng.integers(-149, -126)))  # a denormal a: a24 is exact all the same
        out.append((Fraction(float(a)), Fraction(float(b))))
    return out


def test_the_perm_selectors_on_every_byte_pattern():
    bytes_ = [0x00, 0x01, 0x3C, 0x7F, 0x80, 0xAB, 0xFE, 0xFF]
    seen = 0
    for b3 in bytes_:
        for b2 in bytes_:
            for b1 in bytes_:
                for b0 in range(256):
                    w = (b3 << 24) | (b2 << 16) | (b1 << 8) | b0
                    assert perm(w, w, K_PERM_LO) == (b1 << 16) | b0 and perm(w, w, K_PERM_HI) == (b3 << 16) | b2
                    seen += 1
    for k in range(4):  # every byte position takes all 256 values
        for q in range(256):
            w = (0x5A5A5A5A & ~(0xFF << (8 * k))) | (q << (8 * k))
            pair = perm(w, w, K_PERM_LO if k < 2 else K_PERM_HI)
            assert (pair >> (16 * (k & 1))) & 0xFFFF == q and (pair >> 8) & 0xFF == 0 and pair >> 24 == 0
    assert seen == 8 ** 3 * 256
    # the fallback's halves: the first source is the integer 60, selector bytes 4 picks its low byte
    assert perm(60, 0x04030201, 0x04010400) == 0x3C023C01 and perm(60, 0x04030201, 0x04030402) == 0x3C043C03


def test_the_denormal_form_is_the_fma_bit_for_bit():
    for q in range(256):
        assert half_value(q) == Fraction(q, 1 << 24)
    for a, b in sample():
        a24 = a * (1 << 24)
        assert fl(a24) == a24, "ldexp(a, 24) is exact"
        for q in range(256):
            assert mix(q, a24, b) == fl(q * a + b), (q, float(a), float(b))


def test_the_fallback_form_within_its_bound():
    worst = Fraction(0)
    for a, b in sample(48):
        a1 = a * 1024
        b1 = fl(b - a1)
        for q in range(256):
            assert half_value(0x3C00 | q) == 1 + Fraction(q, 1024)
            t, t1 = fl(q * a + b), mix(0x3C00 | q, a1, b1)
            bound = Fraction(1, 1 << 24) * (abs(b - a1) + abs(t) + abs(t1)) + Fraction(3, 2) * Fraction(2) ** -149  # (+ the denormal quantum, once per rounding)
            assert abs(t1 - t) <= bound, (q, float(a), float(b))
            if a1:
                worst = max(worst, abs(t1 - t) / abs(a1))
    assert worst > 0, "not bit for bit: the form needs wider boxes"


def test_the_scaled_slope_overflows_under_the_old_clamp_only():
    scale = f32(MAX_SCALE)
    a_old = scale * (f32(1.0) / f32(OLD_CLAMP))
    a_new = scale * (f32(1.0) / f32(MIX_CLAMP))
    assert np.isfinite(a_old) and fl(Fraction(float(a_old)) * (1 << 24)) is None  # a is fine, a * 2^24 is not: 0 * inf = NaN for q = 0
    assert fl(Fraction(float(a_new)) * (1 << 24)) == Fraction(2) ** 127
    assert fl(Fraction(float(scale * (f32(1.0) / f32(MIX_CLAMP / 2)))) * (1 << 24)) is None  # 2^-84 is one power of two too small
    # the offsets stay finite as well: |origin|, |o| < 1e8
    assert fl(Fraction(float(f32(1e8))) / Fraction(MIX_CLAMP)) is not None
    # the smallest nonzero direction component a half can hold is far above either clamp: only a zero component is clamped at all
    assert 2.0 ** -24 > 1e6 * max(OLD_CLAMP, MIX_CLAMP)
