"""The NMS suppression predicate, held to exact rational arithmetic on the host.

oracle/yogo_oracle.py:nms_numpy restates torchvision's CPU kernel: a box is suppressed when (double) fl32(inter / uni) > thr.  Here
that predicate is rebuilt WITHOUT a floating-point division (fractions.Fraction, rounded to the nearest float32 by hand) on the
adversarial pairs of tests/_nms_pairs.py, at every scale; the oracle's greedy loop is checked against the keep list the pairs were
constructed to give; the numpy emulation of the kernel's division-free test (nms.hip, THE SUPPRESSION TEST) is checked against the
oracle; and the pair set is shown to tell wrong predicates from the right one, so tests/test_gpu_nms_boundary.py -- which runs the
same images through the kernel -- would notice those errors.
"""
import math

import numpy as np
import pytest
import torch

import _nms_pairs as P
import yogo_oracle as O
from _nms_pairs import THR_BELOW_HALF, THR_F32_UP, THR_JUST_ABOVE_HALF, THRESHOLDS

F32 = np.float32
pytestmark = pytest.mark.filterwarnings("ignore:overflow encountered")


@pytest.fixture(scope="module")
def pairs():
    return P.pair_set()


@pytest.fixture(scope="module")
def terms(pairs):
    """exponent -> (inter, uni, ka, ca) of every pair at that scale"""
    return {e: P.pair_terms(P.scaled(pairs["kept"], e), P.scaled(pairs["cand"], e)) for e in P.SCALE_EXPONENTS}


def test_pair_set_holds_every_class_and_every_scale_regime(pairs, terms):
    n = np.bincount(pairs["cls"], minlength=6)
    print("pairs per class", dict(zip(P.CLASS_NAMES, n.tolist())))
    for c in (P.HALF, P.UP, P.DOWN, P.FAR_BELOW, P.FAR_ABOVE):
        assert n[c] >= 256, (P.CLASS_NAMES[c], int(n[c]))
    assert len(pairs["kept"]) == 2 * P.PAIRS_PER_IMAGE
    assert set(np.unique(pairs["family"])) == {0, 1, 2, 3, 4}
    for f in (0, 1, 2):   # the three drawn families all contribute
        assert (pairs["family"] == f).sum() >= 256
    drawn = pairs["family"] < 3
    assert float(pairs["kept"].max()) <= 4096 and float(pairs["cand"].max()) < P.PITCH
    # both images hold every class
    for img in (0, 1):
        ni = np.bincount(pairs["cls"][P.image_pairs(img)], minlength=6)
        assert (ni[:5] >= 64).all(), (img, ni)
    tiny = float(np.finfo(F32).tiny)
    inter, uni, ka, ca = terms[0]
    assert (uni[drawn] >= 2 ** 13).all() and (uni <= 2 ** 25).all()
    # 2^-45: tiny but normal, every union on the division-free side
    assert ((terms[-45][1] >= P.HANDOVER) & (terms[-45][1] < 2.0 ** -60)).all()
    # the hand-over: one image with at least 64 pairs on each side of union == 2^-100, for the small family (2^-52) and the drawn pairs (2^-61)
    for e, img in ((-52, 1), (-61, 0), (-61, 1)):
        u = terms[e][1][P.image_pairs(img)]
        below, above = int(((u > 0) & (u < P.HANDOVER)).sum()), int((u >= P.HANDOVER).sum())
        print(f"scale 2^{e} image {img}: {below} unions below 2^-100, {int((u == P.HANDOVER).sum())} on it, {above} at or above")
        assert below >= 64 and above >= 64, (e, img, below, above)
    # boundary quotients on both sides of it (an UP / DOWN quotient needs an integer union above 2^24 / 3: 2^-62 puts those below 2^-100)
    for c in (P.HALF, P.UP, P.DOWN):
        u = terms[-62][1]
        assert ((pairs["cls"] == c) & (u > 0) & (u < P.HANDOVER)).sum() >= 64, c
        assert ((pairs["cls"] == c) & (terms[-61][1] >= P.HANDOVER)).sum() >= 64, c
    assert (terms[-52][1] == P.HANDOVER).sum() >= 8
    # the hand-made pair: union exactly 2^-100 at 2^-51, HALF (kept) -- and its sibling (suppressed)
    hand = np.nonzero(pairs["family"] == 4)[0]
    i51, u51 = terms[-51][0][hand], terms[-51][1][hand]
    assert u51[0] == P.HANDOVER and i51[0] == F32(2.0 ** -101) and u51[1] == P.HANDOVER and i51[1] == F32(1.5 * 2.0 ** -101)
    assert P.suppressed(i51, u51, 0.5).tolist() == [False, True]
    # subnormal areas: some at 2^-70, every drawn one at 2^-76
    for e, least in ((-70, 64), (-76, int(drawn.sum()))):
        _, u, ka, ca = terms[e]
        sub = (ka < tiny) & (ca < tiny) & (u < tiny)
        assert sub.sum() >= least and (u[sub] > 0).sum() >= 64, (e, int(sub.sum()))
    assert (terms[-76][2][drawn] < tiny).all() and (terms[-76][3][drawn] < tiny).all()
    # 2^40: finite, the classes unchanged
    assert np.isfinite(terms[40][1]).all() and np.array_equal(P.classify(*terms[40][:2]), pairs["cls"])
    # 2^52: only ka + ca overflows for at least 64 pairs; the union is inf and the pair survives
    inter, uni, ka, ca = terms[52]
    with np.errstate(over="ignore"):
        only_sum = np.isfinite(ka) & np.isfinite(ca) & np.isfinite(inter) & np.isinf(ka + ca)
    assert only_sum.sum() >= 64 and np.isinf(uni[only_sum]).all() and not P.suppressed(inter, uni, 0.5)[only_sum].any()
    assert P.suppressed(inter, uni, 0.5).sum() >= 64   # (and others still are suppressed there)
    # 2^60: both areas of a drawn pair overflow, the union is NaN (inf where the intersection stays finite), nothing is suppressed
    inter, uni, ka, ca = terms[60]
    ovf = np.isinf(ka) & np.isinf(ca)
    assert ovf.sum() >= 1800 and not np.isfinite(uni[ovf]).any() and np.isnan(uni[ovf]).sum() >= 1500
    assert not P.suppressed(inter, uni, 0.5)[drawn].any()


def test_round_fraction_to_f32_known_answers():
    from fractions import Fraction as Fr

    r = P.round_fraction_to_f32
    assert r(Fr(1, 2)) == 0.5 and r(Fr(1, 3)) == float(F32(1) / F32(3)) and r(Fr(-1, 3)) == -float(F32(1) / F32(3))
    assert r(Fr(1, 2) + Fr(1, 2 ** 25)) == 0.5                                 # half way between 0.5 and the next float: to even
    assert r(Fr(1, 2) + Fr(3, 2 ** 25)) == 0.5 + 2.0 ** -23                    # half way, odd below: up
    assert r(Fr(1, 2) + Fr(1, 2 ** 25) + Fr(1, 2 ** 80)) == 0.5 + 2.0 ** -24
    assert r(Fr(1, 2) - Fr(1, 2 ** 26)) == 0.5 and r(Fr(1, 2) - Fr(1, 2 ** 26) - Fr(1, 2 ** 80)) == 0.5 - 2.0 ** -25
    assert r(Fr(1, 2 ** 149)) == 2.0 ** -149 and r(Fr(1, 2 ** 150)) == 0.0 and r(Fr(3, 2 ** 150)) == 2.0 ** -148   # subnormal ties
    assert r(Fr(1, 2 ** 150) + Fr(1, 2 ** 200)) == 2.0 ** -149
    assert r(Fr(2 ** 24 - 1, 2 ** 150)) == 2.0 ** -126                         # rounds up into the normal range
    assert r(Fr(2) ** 128 - Fr(2) ** 103) == math.inf and r(Fr(2) ** 128 - Fr(2) ** 104) == float(np.finfo(F32).max)
    rng = np.random.default_rng(5)
    a = rng.integers(1, 1 << 24, 2000).astype(F32) * F32(2.0) ** rng.integers(-120, 100, 2000).astype(F32)
    b = rng.integers(1, 1 << 24, 2000).astype(F32) * F32(2.0) ** rng.integers(-120, 100, 2000).astype(F32)
    a[:500] = np.ldexp(F32(1), rng.integers(-149, -126, 500)).astype(F32) * rng.integers(1, 9, 500).astype(F32)   # subnormal operands
    with np.errstate(all="ignore"):
        q = a / b
    got = np.asarray([P.exact_quotient(x, y) for x, y in zip(a, b)])
    assert np.array_equal(got, q.astype(np.float64))   # (the host's own fp32 division is correctly rounded too)
    assert (q[np.isfinite(q)] < float(np.finfo(F32).tiny)).sum() > 50 and np.isinf(q).sum() > 5


def test_oracle_predicate_equals_exact_rational_arithmetic(pairs, terms):
    """(double) fl32(inter / uni) > thr with the quotient formed as a Fraction and rounded by hand == what O.nms_numpy decides for the
    pair, at every scale for 0.5 and at the scales of the GPU threshold tests for every threshold used there."""
    N = len(pairs["kept"])
    checked = 0
    for e in P.SCALE_EXPONENTS:
        K, C = P.scaled(pairs["kept"], e), P.scaled(pairs["cand"], e)
        inter, uni, _, _ = terms[e]
        q = np.asarray([P.exact_quotient(inter[i], uni[i]) for i in range(N)])
        for thr in (THRESHOLDS if e in (0, -51) else (0.5,)):
            want = q > thr                                     # NaN: False
            assert np.array_equal(P.suppressed(inter, uni, thr), want), (e, thr)
            # the oracle itself, pair by pair: two boxes, the kept one scored higher; the candidate survives or not
            two = np.stack([K, C], 1)
            scores = np.asarray([1.0, 0.5], dtype=F32)
            step = 1 if thr == 0.5 else 4                      # (every pair at 0.5; every fourth for the other thresholds, all classes in it)
            for i in range(0, N, step):
                keep = O.nms_numpy(two[i], scores, thr)
                assert keep[0] == 0 and (len(keep) == 1) == bool(want[i]), (e, thr, i, two[i].tolist(), q[i])
                checked += 1
    print("pairs checked against O.nms_numpy one by one:", checked)


def test_no_float32_quotient_rounds_down_to_one_half():
    """No pair of float32 values has a quotient in (1/2, 1/2 + 2^-25]: with uni in [2^m, 2^(m+1)), uni / 2 is a multiple of the spacing
    2^(m-24) of the floats around it, so inter > uni / 2 means inter - uni / 2 >= 2^(m-24) > 2^-25 uni.  Hence for a normal union
    `inter - 0.5 uni > 2^-25 uni`, `inter > 0.5 uni` and fl32(inter / uni) > 0.5 are one predicate, and a pair with q == 0.5 has
    inter == uni / 2 exactly.  Checked here on the tightest case: the float just above uni / 2, for unions just below a power of two."""
    rng = np.random.default_rng(11)
    man = np.concatenate([(1 << 24) - 1 - np.arange(4096), rng.integers(1 << 23, 1 << 24, 20000)]).astype(np.int64)
    ex = rng.integers(-123, 100, len(man))
    uni = np.ldexp(man.astype(F32), ex).astype(F32)
    inter = np.nextafter(F32(0.5) * uni, F32(np.inf)).astype(F32)
    assert P.suppressed(inter, uni, 0.5).all()
    assert all(P.exact_quotient(a, b) > 0.5 for a, b in zip(inter[:6000], uni[:6000]))
    assert P.kernel_half_predicate(inter, uni).all() and P.kernel_half_predicate(inter, uni, rhs=False).all()
    assert not P.suppressed(F32(0.5) * uni, uni, 0.5).any()


def test_kernel_division_free_emulation_equals_oracle_predicate(pairs, terms):
    """the numpy-fp32 emulation of nms.hip's test for iou_thresh == 0.5 (big / uni == 0 / odd branches) on every pair and scale"""
    routes = np.zeros(3, dtype=np.int64)
    for e in P.SCALE_EXPONENTS:
        inter, uni, _, _ = terms[e]
        assert np.array_equal(P.kernel_half_predicate(inter, uni), P.suppressed(inter, uni, 0.5)), e
        routes += [int((uni >= P.HANDOVER).sum()), int((uni == 0).sum()), int(((uni > 0) & (uni < P.HANDOVER)).sum())]
    assert (routes > 0).all(), routes   # all three branches were taken
    # and on unions no box pair here produces: negative, NaN, +-inf against every kind of intersection (a product of two max(0, .): never
    # negative -- for a negative intersection over a negative union the two forms do differ).  (A union of -0 is left out: the
    # division-free test reads it as 0 and the quotient as -inf for inter > 0 -- but ka + ca - inter is -0 only when both areas are -0, and
    # a box with a zero extent has inter == 0 or NaN, for which both forms say no.)
    sp = np.asarray([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 2.0 ** -100, 2.0 ** -101, 2.0 ** -149, 2.0 ** -126, 3.0e38], dtype=F32)
    inter, uni = (a.reshape(-1) for a in np.meshgrid(np.delete(sp, [3, 5]), np.delete(sp, 1)))
    assert np.array_equal(P.kernel_half_predicate(inter, uni), P.suppressed(inter, uni, 0.5))
    zero_extent = np.asarray([0.0, -0.0, np.nan], dtype=F32)
    assert not P.kernel_half_predicate(zero_extent, np.full(3, -0.0, dtype=F32)).any()
    assert not P.suppressed(zero_extent, np.full(3, -0.0, dtype=F32), 0.5).any()


def test_pair_set_tells_wrong_predicates_from_the_reference(pairs, terms):
    """each mutant must disagree with the reference on at least one pair that an image of test_gpu_nms_boundary.py holds at a scale
    and threshold it runs -- so a kernel with that slip fails there."""
    cls = pairs["cls"]

    def ref(e, thr=0.5):
        return P.suppressed(terms[e][0], terms[e][1], thr)

    def differs(mutant, scales, thr=0.5, only=None):
        total = 0
        for e in scales:
            d = mutant(e, thr) != ref(e, thr)
            if only is not None:
                assert not d[~only(e)].any()   # the mutant goes wrong where it is meant to and nowhere else
            total += int(d.sum())
        return total

    # (1) `>=` in place of `>` where the quotient is compared (the serial path, the fallback, every threshold but 0.5): the HALF pairs
    ge_div = lambda e, thr: P.quotient(*terms[e][:2]).astype(np.float64) >= thr
    assert differs(ge_div, (0,), only=lambda e: cls == P.HALF) >= 256
    assert differs(ge_div, (-62, -76)) >= 64
    # (in the division-free form `>=` shows only for 0 / 0, two boxes whose areas underflow to zero: inter - 0.5 uni == 2^-25 uni has no
    #  other float32 solution, see (5))
    ge_free = lambda e, thr: P.kernel_half_predicate(*terms[e][:2], ge=True)
    assert differs(ge_free, P.SCALE_EXPONENTS, only=lambda e: (terms[e][1] == 0) & (terms[e][0] == 0)) >= 1
    # (2) the threshold compared in float32: only thresholds that are not float32 values show it
    f32_thr = lambda e, thr: P.quotient(*terms[e][:2]) > F32(thr)
    assert differs(f32_thr, (0, -51), 0.5) == 0
    assert differs(f32_thr, (0, -51), THR_BELOW_HALF, only=lambda e: cls == P.HALF) >= 2 * 256   # float32(thr) == 0.5: HALF no longer suppressed
    assert differs(f32_thr, (0, -51), THR_JUST_ABOVE_HALF) == 0 and F32(THR_JUST_ABOVE_HALF) == F32(0.5)
    # (3) the hand-over bound at 2^-90 with no fallback behind it: unions in (0, 2^-90) never suppress
    no_fb = lambda e, thr: P.kernel_half_predicate(*terms[e][:2], u_lo=F32(2.0 ** -90), fallback=False)
    assert differs(no_fb, (0, -45, 40)) == 0
    assert differs(no_fb, (-52, -61, -62, -70, -76), only=lambda e: (terms[e][1] > 0) & (terms[e][1] < 2.0 ** -90)) >= 256
    # (3b) the division-free form used below its range (no hand-over at all): 2^-25 uni and the difference are no longer exact
    no_lo = lambda e, thr: P.kernel_half_predicate(*terms[e][:2], u_lo=F32(0))
    print("division-free form without a hand-over: wrong on", differs(no_lo, (-70, -76)), "pairs at 2^-70 / 2^-76")
    assert differs(no_lo, (-70, -76)) >= 1
    # (4) subnormals flushed to zero, operands and results
    def ftz(e, thr):
        i, u = P.pair_terms_flushed(P.scaled(pairs["kept"], e), P.scaled(pairs["cand"], e))
        return P.suppressed(P.flush(i), u, thr) & True
    assert differs(ftz, (0, -45, -51, -61, 40, 52, 60)) == 0
    assert differs(ftz, (-70,)) >= 64 and differs(ftz, (-76,)) >= 256
    # (5) the right-hand side 2^-25 uni dropped (inter - 0.5 uni > 0): NOT a wrong predicate.  It is the reference's, for every pair of
    # float32 values (test_no_float32_quotient_rounds_down_to_one_half): no input can tell the two apart, and none here does
    no_rhs = lambda e, thr: P.kernel_half_predicate(*terms[e][:2], rhs=False)
    assert differs(no_rhs, P.SCALE_EXPONENTS) == 0
    # (the slip next to it that can be told apart: `> 2^-24 uni` loses the UP pairs)
    big_rhs = lambda e, thr: (terms[e][0] - F32(0.5) * terms[e][1]) > F32(2.0 ** -24) * terms[e][1]
    assert differs(big_rhs, (0, -45, 40), only=lambda e: cls == P.UP) >= 3 * 256


def _oracle_cells(pred, **kw):
    rows, cells = O.format_preds(torch.from_numpy(pred.copy()), return_cells=True, **kw)
    return rows.numpy(), cells.numpy()


@pytest.mark.parametrize("order", ["interleaved", "split"])
@pytest.mark.parametrize("exponent", [0, -52, -61, -76, 60])
def test_oracle_greedy_loop_returns_the_constructed_keep_list(pairs, exponent, order):
    """O.format_preds on the laid-out images == the keep list built from the pairwise predicate: the oracle's sort and greedy loop against
    the construction (boxes of different pairs never intersect, so nothing else can suppress)"""
    for img in (0, 1):
        idx = P.image_pairs(img)
        im = P.build_image(pairs["kept"][idx], pairs["cand"][idx], exponent, order)
        for fmt in ("cxcywh", "xyxy"):
            rows, cells = _oracle_cells(im["pred"], box_format=fmt)
            assert np.array_equal(cells, im["cells"]), (exponent, order, img, fmt)
            assert np.array_equal(rows.view(np.int32), P.expected_rows(im["pred"], im["cells"], fmt).view(np.int32))
        assert len(im["cells"]) == 2 * len(idx) - int(im["dead"].sum())
        if exponent != 60:
            assert 64 <= im["dead"].sum() <= len(idx) - 64


def test_oracle_keep_list_other_thresholds_and_truncation(pairs):
    idx = P.image_pairs(1)
    for thr in THRESHOLDS[1:]:
        im = P.build_image(pairs["kept"][idx], pairs["cand"][idx], -51, "split", thr=thr)
        rows, cells = _oracle_cells(im["pred"], iou_thresh=thr)
        assert np.array_equal(cells, im["cells"]), thr
    for n in (1, 2, 63, 65, 1025):
        im = P.build_image(pairs["kept"][idx], pairs["cand"][idx], 0, "interleaved", n=n)
        rows, cells = _oracle_cells(im["pred"])
        assert np.array_equal(cells, im["cells"]) and im["n"] == n, n


def test_split_order_reaches_every_owner_wave_and_later_slots():
    """the layout facts the GPU test relies on: n = 2304 (36 chunks, three slots); interleaved pairs share a chunk; split candidates sit
    at least 64 places behind their kept box, in chunks 18 .. 35 (slots 1 and 2, every owner wavefront c & 15)"""
    m = P.PAIRS_PER_IMAGE
    assert 2 * m == 2304 and all((2 * i) // 64 == (2 * i + 1) // 64 for i in range(m))
    chunks = {(m + i) // 64 for i in range(m)}
    assert min(chunks) >= 16 and {c & 15 for c in chunks} == set(range(16)) and {(m + i) // 1024 for i in range(m)} == {1, 2}
    assert {i // 64 & 15 for i in range(m)} == set(range(16))


def test_oracle_threshold_casts_follow_float32():
    """`tensor > python_float` compares in the tensor's dtype: objectness float32(0.3) is NOT above the threshold 0.3, although it is in double"""
    for t in (0.5, 0.3, 0.7):
        c = F32(t)
        vals = np.asarray([np.nextafter(c, F32(0)), c, np.nextafter(c, F32(1))], dtype=F32)
        pred = np.zeros((8, 1, 3), dtype=F32)
        pred[0, 0] = [0.2, 0.5, 0.8]
        pred[1], pred[2], pred[3] = 0.5, 0.1, 0.1
        pred[4, 0] = vals
        pred[5] = 1.0
        rows, cells = _oracle_cells(pred, obj_thresh=t)
        assert cells.tolist() == [2], (t, cells)
        pred[4] = 1.0
        pred[5, 0] = vals
        rows, cells = _oracle_cells(pred, min_class_confidence_threshold=t)
        assert cells.tolist() == [2], (t, cells)
    assert float(F32(0.3)) > 0.3 and float(F32(0.7)) < 0.7
