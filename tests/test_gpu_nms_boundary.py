"""nms.hip at the rounding edges of its suppression test, its thresholds and its sort, on the three routes a pair of boxes can take.

The images come from tests/_nms_pairs.py: pairs of integer boxes whose fp32 quotient inter / union is exactly 0.5, the float above or
below it, or far away, scaled by powers of two down to the kernel's 2^-100 hand-over, into the subnormals and up past the overflow,
and laid out so that a pair meets in the owning wavefront's serial loop (`interleaved`) or in the division-free loop / the division
fallback of a later chunk (`split`).  Counts, cells and the bits of the rows must equal BOTH the keep list the images were
constructed to give (each pair's own predicate; tests/test_nms_predicate_host.py holds that predicate to exact rational arithmetic)
and the CPU algorithm (oracle/yogo_oracle.py:format_preds).
"""
import math

import numpy as np
import pytest
import torch

import _nms_pairs as P
import yogo_oracle as O
from _nms_pairs import THR_BELOW_HALF, THR_F32_UP, THR_JUST_ABOVE_HALF

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered")]

F32 = np.float32


def check(preds, want_cells, **kw):
    """preds: list of [P, Sy, Sx] float32 arrays (one call, B <= 8); want_cells: the constructed kept cells of each, in output order"""
    from yogo_amd.utils import format_preds_batched

    assert len(preds) <= 8
    fmt = kw.get("box_format", "cxcywh")
    batch = torch.from_numpy(np.stack(preds))
    rows, cells, counts = format_preds_batched(batch.cuda(), **kw)
    rows, cells, counts = rows.cpu(), cells.cpu(), counts.cpu()
    assert counts.dtype == torch.int32
    for b, (pred, want) in enumerate(zip(preds, want_cells)):
        n = int(counts[b])
        got_cells, got_rows = cells[b, :n], rows[b, :n].contiguous().view(torch.int32)
        # the construction
        want = torch.from_numpy(np.asarray(want, dtype=np.int64))
        assert n == len(want), (kw, b, n, len(want))
        assert torch.equal(got_cells, want), (kw, b)
        assert torch.equal(got_rows, torch.from_numpy(P.expected_rows(pred, want.numpy(), fmt)).view(torch.int32)), (kw, b)
        # the CPU algorithm
        orows, ocells = O.format_preds(batch[b].clone(), return_cells=True, **kw)
        assert n == orows.shape[0], (kw, b, n, orows.shape[0])
        assert torch.equal(got_cells, ocells), (kw, b)
        assert torch.equal(got_rows, orows.contiguous().view(torch.int32)), (kw, b)
    return rows, cells, counts


def images(exponent, thr=0.5, orders=("interleaved", "split")):
    s = P.pair_set()
    out = []
    for order in orders:
        for img in (0, 1):
            idx = P.image_pairs(img)
            out.append(P.build_image(s["kept"][idx], s["cand"][idx], exponent, order, thr=thr))
    return out


@pytest.mark.parametrize("exponent", P.SCALE_EXPONENTS)
def test_every_route_at_every_scale(exponent):
    """iou_thresh = 0.5: the serial path (interleaved) and the division-free loop with its fallback below 2^-100 (split), all pairs, both
    box formats.  n = 2304 per image: 36 chunks, three register slots, the candidates of `split` in chunks 18 .. 35."""
    ims = images(exponent)
    assert exponent == 60 or all(64 <= im["dead"].sum() <= P.PAIRS_PER_IMAGE - 64 for im in ims)   # both answers occur in every image
    for fmt in ("cxcywh", "xyxy"):
        check([im["pred"] for im in ims], [im["cells"] for im in ims], box_format=fmt)


@pytest.mark.parametrize("thr", [THR_BELOW_HALF, THR_JUST_ABOVE_HALF, THR_F32_UP, 0.25, 0.75],
                         ids=["below_half", "half_plus_2^-30", "float32_above_half", "0.25", "0.75"])
def test_threshold_is_compared_in_double(thr):
    """the double just below 0.5 suppresses the HALF pairs; 0.5 + 2^-30 decides as 0.5 does, through the division for every pair; at the
    float32 above 0.5 the UP pairs survive; 0.25 / 0.75 turn on the FAR pairs.  Integer scale and the 2^-51 images (union 2^-100 pair)."""
    s = P.pair_set()
    inter, uni, _, _ = P.pair_terms(s["kept"], s["cand"])
    at_half = P.suppressed(inter, uni, 0.5)
    now = P.suppressed(inter, uni, thr)
    flipped = s["cls"][at_half != now]
    if thr == THR_BELOW_HALF:
        assert (flipped == P.HALF).all() and len(flipped) >= 256 and now[s["cls"] == P.HALF].all()
    elif thr == THR_JUST_ABOVE_HALF:
        assert len(flipped) == 0
    elif thr == THR_F32_UP:
        assert (flipped == P.UP).all() and len(flipped) >= 256 and not now[s["cls"] == P.UP].any()
    elif thr == 0.25:
        assert len(flipped) >= 64 and not now[s["cls"] == P.FAR_BELOW].any() and now[s["cls"] == P.DOWN].all()
    else:
        assert len(flipped) >= 256 and not now[s["cls"] == P.UP].any() and now[s["cls"] == P.FAR_ABOVE].sum() >= 256
    ims = images(0, thr) + images(-51, thr)
    check([im["pred"] for im in ims], [im["cells"] for im in ims], iou_thresh=thr)


CHUNK_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049)


@pytest.mark.parametrize("ns", [CHUNK_EDGES[:7], CHUNK_EDGES[7:]], ids=["n<=128", "n>=129"])
def test_chunk_and_slot_edges(ns):
    """n candidates around the chunk (64) and register-slot (1024) sizes: the padding of the bitonic sort, the first later candidate
    (jmin), the owner wavefront c & 15 and the slot c >> 4.  The cells that do not fire hold a box that would suppress / be suppressed."""
    s = P.pair_set()
    idx = P.image_pairs(0)
    ims = [P.build_image(s["kept"][idx], s["cand"][idx], 0, "interleaved", n=n) for n in ns]
    for im, n in zip(ims, ns):
        assert im["n"] == n and (n < 64 or im["dead"][: n // 2].any())
    check([im["pred"] for im in ims], [im["cells"] for im in ims])


def _disjoint_image(S=16, C=3):
    """[5 + C, S, S]: one small box in the middle of every cell -- no two intersect"""
    pred = np.zeros((5 + C, S, S), dtype=F32)
    ys, xs = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    pred[0] = ((xs + 0.5) / S).astype(F32)
    pred[1] = ((ys + 0.5) / S).astype(F32)
    pred[2] = pred[3] = F32(0.5 / S)
    return pred


def _by_score(score, keep):
    """cells of `keep` by descending score, NaN first, ties (and +0 / -0) by lower cell"""
    cells = np.nonzero(keep.reshape(-1))[0]
    sc = score.reshape(-1)
    return np.asarray(sorted(cells, key=lambda c: (0, 0.0, c) if math.isnan(sc[c]) else (1, -(float(sc[c]) + 0.0), c)), dtype=np.int64)


@pytest.mark.parametrize("t", [0.5, 0.3, 0.7])
def test_thresholds_are_cast_to_float32(t):
    """obj_thresh / min_class_confidence_threshold arrive as Python floats and are compared as float32(t): a value equal to float32(t) is
    not above it -- also for 0.3, where float32(0.3) > 0.3 in double"""
    c = F32(t)
    vals = np.asarray([np.nextafter(c, F32(0)), c, np.nextafter(c, F32(1)), c - F32(0.2), c + F32(0.2)], dtype=F32)
    cyc = vals[np.arange(256) % 5].reshape(16, 16)
    # objectness on the threshold
    pred = _disjoint_image()
    pred[4] = cyc
    pred[5:] = F32(1.0)
    keep = cyc > c
    assert keep.sum() == 2 * 51 and not keep[cyc == c].any() and (t != 0.3 or (cyc[cyc == c].astype(np.float64) > t).all())
    check([pred], [_by_score(cyc, keep)], obj_thresh=t)
    # the class maximum on the threshold (the maximum moves through the class channels)
    pred = _disjoint_image()
    pred[4] = F32(1.0)
    pred[5:] = F32(-1.0)
    for cell in range(256):
        pred[5 + cell % 3, cell // 16, cell % 16] = cyc[cell // 16, cell % 16]
    check([pred], [_by_score(cyc, keep)], min_class_confidence_threshold=t, box_format="xyxy")


def test_score_order_zeros_ties_subnormals_and_nan():
    """the sort: NaN scores first, +0 and -0 equal, equal scores and signed zeros in cell order, subnormal scores in their place"""
    sub = F32(1e-40)
    assert 0 < sub < np.finfo(F32).tiny
    vals = np.asarray([0.0, -0.0, 0.5, 0.5, sub, -sub, np.nan, 0.25, -0.5, 0.5, 2 * sub], dtype=F32)
    score = vals[np.arange(256) % len(vals)].reshape(16, 16)
    pred = _disjoint_image()
    pred[4] = F32(1.0)
    pred[5:] = score                                 # every class channel the same value ...
    nan = np.isnan(score)
    pred[5][nan], pred[7][nan] = F32(0.3), F32(0.9)  # ... and a NaN score from ONE NaN class value among larger and smaller ones
    want = _by_score(score, np.ones_like(score, dtype=bool))
    assert np.isnan(score.reshape(-1)[want[:23]]).all() and (np.diff(want[:23]) > 0).all()
    rows, cells, counts = check([pred], [want], box_format="xyxy")
    assert int(counts[0]) == 256


def test_same_input_same_bits():
    ims = images(-61, orders=("split",))
    from yogo_amd.utils import format_preds_batched

    x = torch.from_numpy(np.stack([im["pred"] for im in ims])).cuda()
    a = format_preds_batched(x)
    b = format_preds_batched(x)
    assert torch.equal(a[2], b[2])
    for i, n in enumerate(a[2].tolist()):
        assert n == len(ims[i]["cells"])
        assert torch.equal(a[1][i, :n], b[1][i, :n]) and torch.equal(a[0][i, :n].view(torch.int32), b[0][i, :n].view(torch.int32))
