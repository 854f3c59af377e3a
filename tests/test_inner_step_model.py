"""A numpy model of the inner step's bookkeeping as the comments of csrc/rt_device.h: trav_inner<true> and DESIGN.md §5 state it.

The one-launch kernels hold "this child was hit" as four lane masks; k_wf_finish gives a missed child no key at all, k_megakernel keeps
its +inf key for the swaps only. The model runs the three comparators each way — on +inf keys with `< inf` tests, as the other traversal
kernels still do, and on the masks in both forms — with one lane per case, so a numpy bool array IS a lane mask and the algebra below is
the kernel's, operation for operation.

The second half is about a compare the kernel does NOT use: the near clamp max(n, 0) folded into a signed-integer compare of the floats'
bit patterns. The two differ only behind the origin, exactly as stated below — and one of those differences is why it was not built: an
absent child's inverted box (qlo = 255, qhi = 0) behind the origin passes the integer compare, and its child word is the end-of-traversal
sentinel."""
import itertools

import numpy as np

f32 = np.float32
INF = f32(np.inf)
K_T_NEAR = f32(1e-4)
CE = ((0, 1), (2, 3), (0, 2))  # the comparators, in order


def cases():
    """hit patterns x key vectors, one lane each: all 16 patterns of four children; keys from {1, 2, 3, 4}^4, which holds every order of
    four distinct keys, every pattern of two, three and four equal keys and every placement of them"""
    keys = np.array(list(itertools.product((1.0, 2.0, 3.0, 4.0), repeat=4)), f32)
    pats = np.array(list(itertools.product((False, True), repeat=4)))
    k = np.repeat(keys, len(pats), axis=0)
    h = np.tile(pats, (len(keys), 1))
    return k, h


def sort_on_inf_keys(key, hit):
    """K = hit ? tn : +inf; a comparator swaps iff KB < KA and moves key and child; afterwards every slot is asked `< inf` on its own"""
    k = [np.where(hit[:, i], key[:, i], INF) for i in range(4)]
    c = [np.full(len(key), i) for i in range(4)]
    for a, b in CE:
        sw = k[b] < k[a]
        k[a], k[b] = np.where(sw, k[b], k[a]), np.where(sw, k[a], k[b])
        c[a], c[b] = np.where(sw, c[b], c[a]), np.where(sw, c[a], c[b])
    return np.stack(c, 1), k[0] < INF, [k[i] < INF for i in (1, 2, 3)]


def sort_on_masks(key, hit, miss_key, miss_keys=False):
    """sw = hB & (~hA | lanes(KB < KA)); the key of the minimum slot and both children move on sw; hA' = hA | hB, hB' = hA & hB.
    `miss_key` stands in every missed child's key: nothing may depend on it. miss_keys (trav_inner<true, true>, k_megakernel): a miss keeps
    its +inf key and sw is the bare compare; the masks still decide `descend` and the pushes."""
    k = [np.where(hit[:, i], key[:, i], INF if miss_keys else miss_key) for i in range(4)]
    h = [hit[:, i].copy() for i in range(4)]
    c = [np.full(len(key), i) for i in range(4)]
    for a, b in CE:
        with np.errstate(invalid="ignore"):
            sw = (k[b] < k[a]) if miss_keys else h[b] & (~h[a] | (k[b] < k[a]))
        k[a] = np.where(sw, k[b], k[a])  # the maximum's key is written nowhere: nothing reads it
        c[a], c[b] = np.where(sw, c[b], c[a]), np.where(sw, c[a], c[b])
        h[a], h[b] = h[a] | h[b], h[a] & h[b]
    return np.stack(c, 1), h[0], [h[1], h[2], h[3]]


def test_the_mask_algebra_orders_descends_and_pushes_as_the_inf_keys_do():
    key, hit = cases()
    assert len(key) == 256 * 16
    assert len({tuple(r) for r in key if len(set(r)) == 4}) == 24  # every order of four distinct keys
    order, descend, pushes = sort_on_inf_keys(key, hit)
    for miss_key, miss_keys in ((f32(-1e30), False), (f32(0.0), False), (INF, False), (f32(np.nan), False), (INF, True)):
        o, d, p = sort_on_masks(key, hit, miss_key, miss_keys)  # (what a missed child's key holds must not matter)
        what = f"miss key {miss_key}, kept {miss_keys}"
        np.testing.assert_array_equal(o, order, err_msg=f"child order, {what}")
        np.testing.assert_array_equal(d, descend, err_msg=f"descend, {what}")
        for slot, (got, want) in enumerate(zip(p, pushes), 1):
            np.testing.assert_array_equal(got, want, err_msg=f"push of slot {slot}, {what}")
    # and the bookkeeping means what the step takes it to mean
    n_hit = hit.sum(1)
    np.testing.assert_array_equal(descend, n_hit > 0)
    np.testing.assert_array_equal(descend.astype(int) + sum(p.astype(int) for p in pushes), n_hit)
    lanes = np.arange(len(key))
    first = order[:, 0]
    assert hit[lanes, first][descend].all()  # the child descended into was hit ...
    nearest = np.where(hit, key, INF).min(1)
    np.testing.assert_array_equal(key[lanes, first][descend], nearest[descend])  # ... and no hit child is nearer
    for slot, p in enumerate(pushes, 1):
        assert hit[lanes, order[:, slot]][p].all()  # a pushed slot holds a hit child


def test_a_comparator_on_masks_never_reads_the_key_of_a_miss():
    """both missed: no swap; only B hit: swap; only A hit: none — whatever the keys are"""
    for ka, kb in itertools.product((f32(1), f32(2), INF, f32(np.nan), f32(-5)), repeat=2):
        for ha, hb, want in ((False, False, False), (False, True, True), (True, False, False)):
            with np.errstate(invalid="ignore"):
                assert (hb and (not ha or bool(kb < ka))) == want


# ---- the near clamp in the compare: what it would change ------------------------------------------------------------------------------------
def as_i32(x):
    return np.asarray(x, f32).view(np.int32)


def clamped(n, f):
    return np.maximum(n, f32(0)) <= f  # the kernels' test


def on_bits(n, f):
    return as_i32(n) <= as_i32(f)  # the floats' bit patterns as signed integers, n unclamped


def crafted():
    denorm = np.array([1], np.uint32).view(f32)[0]
    huge = f32(3e38)
    vals = np.array([0.0, -0.0, denorm, -denorm, K_T_NEAR, -K_T_NEAR, 1.0, -1.0, huge, -huge], f32)
    n, f = np.meshgrid(vals, np.append(vals, INF), indexing="ij")
    return n.ravel(), f.ravel()


def test_the_compare_on_bit_patterns_equals_the_clamped_one_in_front_of_the_origin():
    n, f = crafted()
    front = ~np.signbit(f)  # f >= +0
    assert front.sum() == 10 * 6
    np.testing.assert_array_equal(on_bits(n, f)[front], clamped(n, f)[front])


def test_behind_the_origin_the_two_compares_differ_on_exactly_this_set():
    n, f = crafted()
    behind = np.signbit(f)
    a, b = clamped(n, f), on_bits(n, f)
    neg_zero_n = np.signbit(n) & (n == 0)
    # f == -0.0: the clamped test says 0 <= -0.0 for every n <= 0, the integer one only for n == -0.0 (the box ends at t = 0 < kTNear)
    lost = behind & (f == 0) & (n <= 0) & ~neg_zero_n
    # f < 0: the clamped test never passes; the integer one passes where n carries a sign and n >= f as floats — a box the ray's LINE misses
    # (or of no depth), wholly behind the origin
    gained = behind & (f < 0) & np.signbit(n) & (n >= f)
    assert lost.sum() > 0 and gained.sum() > 0
    np.testing.assert_array_equal(a & ~b, lost)
    np.testing.assert_array_equal(b & ~a, gained)


def test_an_absent_childs_box_behind_the_origin_passes_the_compare_on_bit_patterns():
    """Why the kernel keeps the clamp. An absent child is stored as an inverted box (qlo = 255, qhi = 0: entry > exit on every axis) and
    needs no test of its own BECAUSE max(n, 0) <= f fails on it for every ray. With the origin beyond the node on all three axes both n and
    f are negative with n > f, which is the `gained` set above: the child would count as hit. Its word is kChildEmpty == kTravDone — a lane
    that descends into it, or pops it, ends its traversal with live entries still on its stack — and the builder's stack bound counts
    present children only."""
    scale, origin = f32(1.0 / 64.0), f32(0.0)
    for o, d in ((f32(10.0), f32(1.0)), (f32(-10.0), f32(-1.0))):  # the ray leaves the node behind, either direction sign
        inv = f32(1.0) / d
        a, b = f32(scale * inv), f32(origin * inv - o * inv)
        q_near, q_far = (f32(255), f32(0)) if d > 0 else (f32(0), f32(255))  # the near plane word is qlo for a positive direction, qhi otherwise
        n, f = f32(q_near * a + b), f32(q_far * a + b)
        assert f < n < 0
        assert not clamped(n, f)
        assert on_bits(n, f)
