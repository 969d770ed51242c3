"""Adversarial box pairs for the NMS suppression test (yogo_amd/csrc/nms.hip, "THE SUPPRESSION TEST"), host only, numpy.

A PAIR is a kept box and a lower-scored candidate.  Both have integer xyxy coordinates <= 4096 (so every difference, and every
product up to 2^24, is exact in fp32), and a pair is classified by what the CPU algorithm computes for it in fp32, in the oracle's
operation order (oracle/yogo_oracle.py:nms_numpy): areas from x2 - x1, inter = max(0, .) * max(0, .), uni = ka + ca - inter,
q = fl32(inter / uni).  The classes sit where a wrong comparison shows: q exactly 0.5 (HALF), the float above (UP) and below (DOWN)
it, and far away on either side.

Scaling every coordinate by a power of two is exact, areas scale by its square, and q does not change until something overflows or
goes subnormal: the same pairs are laid out at scales that put the union at the kernel's 2^-100 hand-over, into the subnormals
and past the overflow.  `build_image` lays pairs out in a [5 + C, 48, 48] prediction so that a pair meets in the kernel's serial
path (`interleaved`) or in its division-free loop / division fallback (`split`); pairs are translated apart, so the expected keep
list follows from each pair's own predicate and from nothing else.
"""
import functools
from fractions import Fraction

import numpy as np

F32 = np.float32
HALF, UP, DOWN, FAR_BELOW, FAR_ABOVE, OTHER = range(6)
CLASS_NAMES = ("HALF", "UP", "DOWN", "FAR_BELOW", "FAR_ABOVE", "OTHER")
Q_UP = np.nextafter(F32(0.5), F32(1))
Q_DOWN = np.nextafter(F32(0.5), F32(0))

GRID = 48                 # 48 x 48 cells, every one firing: n = 2304 = 36 chunks of 64, three register slots per lane
PAIRS_PER_IMAGE = GRID * GRID // 2
NUM_CLASSES = 3
PITCH = 8192              # pairs sit on a PITCH lattice (every box lies inside [0, PITCH) before translation)
PER_CLASS = 400           # drawn pairs per class (the issue asks for >= 256)

# coordinate scales (areas scale by the square).  With integer unions between 2^13 and 2^25 for the drawn pairs:
#   2^0    the integers themselves
#   2^-45  unions 2^-77 .. 2^-65: tiny, far inside the normal range, all on the division-free test
#   2^-51  the hand-made pair with union EXACTLY 2^-100 (integer union 4) and the small family around it
#   2^-52  integer union 16 is 2^-100: the small family straddles the hand-over
#   2^-61  the drawn pairs straddle the hand-over (integer union 2^22 is 2^-100): boundary quotients on both routes
#   2^-62  the same with integer union 2^24 at the hand-over
#   2^-70  area scale 2^-140: subnormal or zero areas for boxes below 2^14 integer area (the small family)
#   2^-76  area scale 2^-152: every drawn area is subnormal (<= 2^25 2^-152 < 2^-126)
#   2^40   large and finite
#   2^52   areas < 2^128 but ka + ca overflows for boxes of 2^23 .. 2^24 integer area: uni = inf, q = 0
#   2^60   areas overflow: uni = inf + inf - inf = NaN, nothing is suppressed
SCALE_EXPONENTS = (0, -45, -51, -52, -61, -62, -70, -76, 40, 52, 60)
HANDOVER = F32(2.0 ** -100)

# the IoU thresholds of the tests (Python floats, i.e. doubles)
THR_BELOW_HALF = float(np.nextafter(0.5, 0.0))                    # the double below 0.5: q == 0.5 is now suppressed
THR_JUST_ABOVE_HALF = 0.5 + 2.0 ** -30                            # not a float32: decides as 0.5 does, but never by the division-free form
THR_F32_UP = float(np.nextafter(F32(0.5), F32(1)))                # the float32 above 0.5: q == that float is NOT suppressed
THRESHOLDS = (0.5, THR_BELOW_HALF, THR_JUST_ABOVE_HALF, THR_F32_UP, 0.25, 0.75)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 arithmetic of one pair, in the oracle's order
# ---------------------------------------------------------------------------------------------------------------------
def scaled(boxes, e):
    """boxes * 2^e in fp32 (exact: a power of two, and no coordinate here leaves the normal range)"""
    return np.ldexp(np.asarray(boxes, dtype=F32), e).astype(F32)


def pair_terms(kept, cand):
    """fp32 (inter, uni, ka, ca) of kept[i] against cand[i]; [N, 4] xyxy each"""
    kept = np.asarray(kept, dtype=F32)
    cand = np.asarray(cand, dtype=F32)
    with np.errstate(all="ignore"):
        ka = (kept[:, 2] - kept[:, 0]) * (kept[:, 3] - kept[:, 1])
        ca = (cand[:, 2] - cand[:, 0]) * (cand[:, 3] - cand[:, 1])
        xx1 = np.maximum(kept[:, 0], cand[:, 0])
        yy1 = np.maximum(kept[:, 1], cand[:, 1])
        xx2 = np.minimum(kept[:, 2], cand[:, 2])
        yy2 = np.minimum(kept[:, 3], cand[:, 3])
        w = np.maximum(F32(0), xx2 - xx1)
        h = np.maximum(F32(0), yy2 - yy1)
        inter = w * h
        uni = ka + ca - inter
    assert inter.dtype == F32 and uni.dtype == F32
    return inter, uni, ka, ca


def quotient(inter, uni):
    with np.errstate(all="ignore"):
        q = inter / uni
    assert q.dtype == F32
    return q


def suppressed(inter, uni, thr):
    """the reference predicate: (double) fl32(inter / uni) > thr, thr a Python float (double)"""
    with np.errstate(all="ignore"):
        return quotient(inter, uni).astype(np.float64) > float(thr)


def classify(inter, uni):
    q = quotient(inter, uni)
    cls = np.full(q.shape, OTHER, dtype=np.int64)
    with np.errstate(all="ignore"):
        cls[inter < F32(0.25) * uni] = FAR_BELOW
        cls[q >= F32(0.75)] = FAR_ABOVE
    cls[q == F32(0.5)] = HALF
    cls[q == Q_UP] = UP
    cls[q == Q_DOWN] = DOWN
    return cls


# ---------------------------------------------------------------------------------------------------------------------
# exact rational arithmetic: fl32(inter / uni) without a floating-point division
# ---------------------------------------------------------------------------------------------------------------------
def round_fraction_to_f32(fr):
    """nearest float32 of a Fraction, ties to even, subnormal results and overflow included; returned as a Python float"""
    if fr == 0:
        return 0.0
    sign = -1.0 if fr < 0 else 1.0
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()   # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    qexp = max(e, -126) - 23                                     # the spacing of float32 around a (subnormals: 2^-149)
    n = a / Fraction(2) ** qexp
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (lo & 1)):
        lo += 1
    val = Fraction(lo) * Fraction(2) ** qexp
    if val >= Fraction(2) ** 128:
        return sign * float("inf")
    return sign * float(val)


def exact_quotient(inter, uni):
    """what a correctly rounded fp32 division returns for two float32 values, IEEE special cases written out"""
    inter, uni = float(inter), float(uni)
    nan, inf = float("nan"), float("inf")
    if inter != inter or uni != uni:
        return nan
    if abs(inter) == inf:
        return nan if abs(uni) == inf else (inter if np.copysign(1.0, uni) > 0 else -inter)
    if abs(uni) == inf:
        return 0.0 * np.copysign(1.0, inter) * np.copysign(1.0, uni)
    if uni == 0.0:
        return nan if inter == 0.0 else np.copysign(inf, inter) * np.copysign(1.0, uni)
    if inter == 0.0:
        return 0.0 * np.copysign(1.0, inter) * np.copysign(1.0, uni)
    return round_fraction_to_f32(Fraction(inter) / Fraction(uni))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's predicate for iou_thresh == 0.5, emulated in numpy fp32 (nms.hip: the division-free loop and its fallback)
# ---------------------------------------------------------------------------------------------------------------------
def kernel_half_predicate(inter, uni, u_lo=HANDOVER, rhs=True, fallback=True, ge=False):
    """dead |= (big || uni == 0) && (inter - 0.5f * uni > 0x1p-25f * uni);  odd |= uni > 0 && !big  -> the division for the odd ones.
    The keyword arguments switch in the mutants of tests/test_nms_predicate_host.py."""
    inter = np.asarray(inter, dtype=F32)
    uni = np.asarray(uni, dtype=F32)
    with np.errstate(all="ignore"):
        big = uni >= F32(u_lo)
        lhs = inter - F32(0.5) * uni
        r = F32(2.0 ** -25) * uni if rhs else np.zeros_like(uni)
        assert lhs.dtype == F32 and r.dtype == F32
        cmp = (lhs >= r) if ge else (lhs > r)
        dead = (big | (uni == F32(0))) & cmp
        odd = (uni > F32(0)) & ~big
        if fallback:
            dead = dead | (odd & ((inter / uni).astype(np.float64) > 0.5))
    return dead


def flush(x):
    """subnormal float32 values -> signed zero (what a flushing route would see)"""
    x = np.asarray(x, dtype=F32).copy()
    sub = (np.abs(x) < np.finfo(F32).tiny) & (x != 0)
    x[sub] = np.copysign(F32(0), x[sub])
    return x


def pair_terms_flushed(kept, cand):
    """pair_terms with every operand and result flushed to zero when subnormal"""
    kept = flush(kept)
    cand = flush(cand)
    with np.errstate(all="ignore"):
        ka = flush((kept[:, 2] - kept[:, 0]) * (kept[:, 3] - kept[:, 1]))
        ca = flush((cand[:, 2] - cand[:, 0]) * (cand[:, 3] - cand[:, 1]))
        w = np.maximum(F32(0), np.minimum(kept[:, 2], cand[:, 2]) - np.maximum(kept[:, 0], cand[:, 0]))
        h = np.maximum(F32(0), np.minimum(kept[:, 3], cand[:, 3]) - np.maximum(kept[:, 1], cand[:, 1]))
        inter = flush(flush(w) * flush(h))
        uni = flush(flush(ka + ca) - inter)
    return inter, uni


# ---------------------------------------------------------------------------------------------------------------------
# the pair set
# ---------------------------------------------------------------------------------------------------------------------
def _draw_families(rng, n):
    """n draws of each family -> (kept [3n, 4], cand [3n, 4], family [3n]) as int64"""
    z = np.zeros(n, dtype=np.int64)
    # family 0: kept [0, 0, W, H], candidate [x, 0, x + w, H] with x ~ W/3 and w ~ W: inter / uni = (W - x) / (x + w) ~ 1/2
    W = rng.integers(1536, 4093, n)
    H = rng.integers(1536, 4097, n)
    x = (W + 1) // 3 + rng.integers(-2, 3, n)
    w = W + rng.integers(-2, 3, n)
    k0 = np.stack([z, z, W, H], 1)
    c0 = np.stack([x, z, x + w, H], 1)
    # family 1: candidate nested in the kept box: inter / uni = w h / (W H).  A third of the draws at h ~ H/2, full width (quotient ~ 1/2),
    # the rest anywhere inside
    W = rng.integers(64, 4097, n)
    H = rng.integers(64, 4097, n)
    near = rng.random(n) < 1 / 3
    w = np.where(near, W, np.maximum(1, (W * rng.random(n) ** 0.5).astype(np.int64)))
    h = np.where(near, np.clip(H // 2 + rng.integers(-2, 3, n), 1, H), np.maximum(1, (H * rng.random(n) ** 0.5).astype(np.int64)))
    a = ((W - w + 1) * rng.random(n)).astype(np.int64)
    b = ((H - h + 1) * rng.random(n)).astype(np.int64)
    k1 = np.stack([z, z, W, H], 1)
    c1 = np.stack([a, b, a + w, b + h], 1)
    # family 2: offset along both axes, sizes within a few cells of each other
    W = rng.integers(64, 3000, n)
    H = rng.integers(64, 3000, n)
    dx = (W * rng.random(n)).astype(np.int64)
    dy = (H * rng.random(n)).astype(np.int64)
    w = np.maximum(1, W + rng.integers(-3, 4, n))
    h = np.maximum(1, H + rng.integers(-3, 4, n))
    k2 = np.stack([z, z, W, H], 1)
    c2 = np.stack([dx, dy, dx + w, dy + h], 1)
    fam = np.repeat(np.arange(3), n)
    return np.concatenate([k0, k1, k2]), np.concatenate([c0, c1, c2]), fam


def _small_family():
    """every kept [0, 0, W, H] / candidate [x, 0, x + w, H] with tiny integers whose integer union lies in [8, 32): at the coordinate
    scale 2^-52 the union 16 is exactly the 2^-100 hand-over, so this family sits on both sides of it and on it"""
    out_k, out_c = [], []
    for H in (1, 2, 3):
        for W in range(1, 17):
            for x in range(0, W):
                for w in range(1, 17):
                    uni = max(W, x + w) * H
                    if 8 <= uni < 32:
                        out_k.append((0, 0, W, H))
                        out_c.append((x, 0, x + w, H))
    return np.asarray(out_k, dtype=np.int64), np.asarray(out_c, dtype=np.int64)


# the hand-made pair: integer union 4, so 2^-100 exactly at the coordinate scale 2^-51 (HALF: not suppressed), and its sibling (q = 0.75)
HAND_KEPT = np.asarray([(0, 0, 2, 1), (0, 0, 3, 1)], dtype=np.int64)
HAND_CAND = np.asarray([(0, 0, 4, 1), (0, 0, 4, 1)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def pair_set(seed=20240611):
    """-> dict(kept [N, 4] float32, cand [N, 4] float32, cls [N], family [N]); N = 2 * PAIRS_PER_IMAGE.

    Order: image 0 = pairs [0, 1152) -- drawn pairs only; image 1 = pairs [1152, 2304) -- the rest of the drawn pairs, then the small
    family (a deterministic sample of it), then the two hand-made pairs.  The classes are interleaved, so each image holds all five.
    family: 0 / 1 / 2 drawn (see _draw_families), 3 small, 4 hand-made."""
    rng = np.random.default_rng(seed)
    kept, cand, fam = _draw_families(rng, 1 << 20)
    ok = (cand[:, 2] < PITCH) & (cand[:, 3] < PITCH) & (kept.max(1) <= 4096) & ((cand[:, 2] - cand[:, 0]) <= 4096) & ((cand[:, 3] - cand[:, 1]) <= 4096)
    kept, cand, fam = kept[ok], cand[ok], fam[ok]
    inter, uni, _, _ = pair_terms(kept, cand)
    cls = classify(inter, uni)
    picks = []
    for c in (HALF, UP, DOWN, FAR_BELOW, FAR_ABOVE):
        idx = np.nonzero(cls == c)[0]
        # (every HALF pair has inter == uni / 2 exactly: no float32 quotient lies in (1/2, 1/2 + 2^-25], see test_nms_predicate_host.py)
        if c == FAR_BELOW:
            idx = idx[inter[idx] > 0]          # disjoint boxes teach nothing
        # PER_CLASS of them, spread over the families, in drawing order
        byfam = [idx[fam[idx] == f] for f in range(3)]
        chosen, r = [], 0
        while len(chosen) < PER_CLASS and any(r < len(b) for b in byfam):
            chosen += [b[r] for b in byfam if r < len(b)]
            r += 1
        chosen = chosen[:PER_CLASS]
        picks.append(np.asarray(chosen, dtype=np.int64))
    n_drawn = sum(len(p) for p in picks)
    # interleave the classes
    order = []
    for r in range(max(len(p) for p in picks)):
        order += [p[r] for p in picks if r < len(p)]
    order = np.asarray(order, dtype=np.int64)
    sk, sc = _small_family()
    n_small = 2 * PAIRS_PER_IMAGE - n_drawn - len(HAND_KEPT)
    assert 0 < n_small <= len(sk), (n_small, len(sk), n_drawn)
    sel = np.round(np.linspace(0, len(sk) - 1, n_small)).astype(np.int64)
    assert len(np.unique(sel)) == n_small
    K = np.concatenate([kept[order], sk[sel], HAND_KEPT]).astype(F32)
    C = np.concatenate([cand[order], sc[sel], HAND_CAND]).astype(F32)
    family = np.concatenate([fam[order], np.full(n_small, 3), np.full(len(HAND_KEPT), 4)])
    i2, u2, _, _ = pair_terms(K, C)
    out = dict(kept=K, cand=C, cls=classify(i2, u2), family=family)
    for v in out.values():
        v.setflags(write=False)
    return out


def image_pairs(image):
    """indices into pair_set() of the pairs of image 0 / 1"""
    return np.arange(image * PAIRS_PER_IMAGE, (image + 1) * PAIRS_PER_IMAGE)


# ---------------------------------------------------------------------------------------------------------------------
# layout into a prediction tensor
# ---------------------------------------------------------------------------------------------------------------------
def build_image(kept, cand, exponent, order, thr=0.5, n=None, seed=7):
    """kept / cand [m, 4] integer xyxy (float32), m <= 1152 -> dict(pred [5 + C, 48, 48] float32 cxcywh, cells, keep_rank, n).

    Box r of the sorted order gets class value (4096 - r) / 4096 (exact, distinct, descending) and objectness 1, in a pseudo-random cell.
    order = "interleaved": kept box i at rank 2 i, its candidate at 2 i + 1 (same 64-chunk: the serial path);
    order = "split": kept boxes at ranks [0, m), candidates at [m, 2 m) (m >= 64: a later chunk -- the division-free loop / the fallback).
    n (interleaved only) keeps the first n ranks; every other cell holds a copy of rank 0's box with objectness 0.25 (below any
    threshold used: were it a candidate, it would be suppressed or suppress).
    `cells` are the kept cells in output order and `keep_rank` their ranks, from each pair's own predicate at threshold `thr`."""
    kept = np.asarray(kept, dtype=F32)
    cand = np.asarray(cand, dtype=F32)
    m = len(kept)
    assert m == len(cand) and 2 * m <= GRID * GRID
    i = np.arange(m)
    off = np.stack([(i % 32) * PITCH, (i // 32) * PITCH], 1).astype(F32)
    off = np.concatenate([off, off], 1)
    assert float((cand + off).max()) < 2 ** 23
    tk, tc = scaled(kept + off, exponent), scaled(cand + off, exponent)
    inter, uni, _, _ = pair_terms(scaled(kept, exponent), scaled(cand, exponent))
    dead = suppressed(inter, uni, thr)
    if order == "interleaved":
        boxes = np.empty((2 * m, 4), dtype=F32)
        boxes[0::2], boxes[1::2] = tk, tc
        alive = np.ones(2 * m, dtype=bool)
        alive[1::2] = ~dead
    else:
        assert order == "split" and m >= 64 and n is None
        boxes = np.concatenate([tk, tc])
        alive = np.concatenate([np.ones(m, dtype=bool), ~dead])
    n = 2 * m if n is None else n
    assert 1 <= n <= 2 * m
    boxes, alive = boxes[:n], alive[:n]
    cell_of_rank = np.random.default_rng(seed).permutation(GRID * GRID)
    pred = np.zeros((5 + NUM_CLASSES, GRID * GRID), dtype=F32)
    with np.errstate(over="ignore"):
        cx = (boxes[:, 0] + boxes[:, 2]) / F32(2)
        cy = (boxes[:, 1] + boxes[:, 3]) / F32(2)
    bw = boxes[:, 2] - boxes[:, 0]
    bh = boxes[:, 3] - boxes[:, 1]
    # the kernel's (and torchvision's) cx -+ 0.5 w must give the scaled integers back
    assert np.array_equal(cx - F32(0.5) * bw, boxes[:, 0]) and np.array_equal(cx + F32(0.5) * bw, boxes[:, 2])
    assert np.array_equal(cy - F32(0.5) * bh, boxes[:, 1]) and np.array_equal(cy + F32(0.5) * bh, boxes[:, 3])
    # filler for the cells that do not fire: rank 0's box
    pred[0], pred[1], pred[2], pred[3] = cx[0], cy[0], bw[0], bh[0]
    pred[4] = F32(0.25)
    pred[5] = F32(1.0)
    cells = cell_of_rank[:n]
    pred[0, cells], pred[1, cells], pred[2, cells], pred[3, cells] = cx, cy, bw, bh
    pred[4, cells] = F32(1.0)
    pred[5, cells] = ((4096 - np.arange(n)) / 4096).astype(F32)
    keep_rank = np.nonzero(alive)[0]
    return dict(pred=pred.reshape(5 + NUM_CLASSES, GRID, GRID), cells=cells[keep_rank].astype(np.int64), keep_rank=keep_rank, n=n,
                dead=dead)


def expected_rows(pred, cells, box_format):
    """the rows format_preds returns for the kept cells: the prediction's columns, the box converted in fp32 for xyxy"""
    flat = pred.reshape(pred.shape[0], -1)
    rows = flat[:, cells].T.copy()
    if box_format == "xyxy":
        cx, cy, w, h = (rows[:, k].copy() for k in range(4))
        rows[:, 0] = cx - F32(0.5) * w
        rows[:, 1] = cy - F32(0.5) * h
        rows[:, 2] = cx + F32(0.5) * w
        rows[:, 3] = cy + F32(0.5) * h
    return rows
