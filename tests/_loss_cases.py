"""Edge cases for the decode and loss kernels (yogo_amd/csrc/decode_loss.hip; their arithmetic: head_math.h), their references and a numpy transcription.  Host only.

CASES.  Every box corner is dyadic (a multiple of 2^-6, scaled by 2^-k about a dyadic anchor), so corners, clamps and comparisons are
exact in float32 AND float64: both precisions take the same branch at every `max` / `min` tie, clamp mask, `has` predicate and exp
clamp (tests/test_loss_edges_host.py checks that with nothing left out).  The one decision that float64 cannot reproduce -- the
reference's float32 zero-area filter x1 != x2 (yogo_loss.py:84-90) -- is handed to the float64 reference from float32 arithmetic.
A GROUP is a list of cells that share P and the four loss weights (launch parameters); RAW is the group of head outputs for the
decode and the fused decode + loss + decode-backward kernel.

REFERENCES.  `ref_cells` evaluates the oracle's own functions (O.box_convert_cxcywh_to_xyxy, torch.clamp, O.complete_box_iou_loss,
F.cross_entropy, F.mse_loss, O.decode) per cell with torch autograd, in float64 (`ref64`) and float32 (`ref32`, what the kernel
imitates).  Nothing comes from the code under test.  Scale of a cell: s = max(max_c |ref32 - ref64|, ulp32(max_c |ref64|)); a kernel
is held to |kernel - ref64| <= M s  (M: tests/_util.py LOSS_EDGE_M).

TRANSCRIPTION.  `k_loss`, `k_decode`, `k_decode_bwd` restate the kernels' per-cell statements (the functions of head_math.h in the order
the kernels call them) in numpy float32 (no fused multiply-add, as their translation units are built with -ffp-contract=off).  `var` switches in the wrong variants that the host test must reject.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import yogo_oracle as O

F32 = np.float32
EPS = 1e-7
DEFAULT_W = (0.5, 5.0, 1.0, 0.01)        # no_obj_weight, iou_weight, classify_weight, label_smoothing
GRID = (17, 19)                           # Sy, Sx of the packed batches: 323 cells = one workgroup + 67 lanes (a partial wavefront)
ANCHORS = (0.0425, 0.0555, 1.5, 0.75)     # anchor_w, anchor_h, width_multiplier, height_multiplier of the raw-level cases
G0 = (16, 20, 40, 52)                     # the usual label box, in 1/64


class Group:
    def __init__(self, name, pred, label, fam, w=DEFAULT_W, hp0=None):
        self.name, self.w = name, tuple(float(v) for v in w)
        self.pred = np.ascontiguousarray(pred, dtype=F32)      # [N, 5 + C]  cx, cy, w, h, objectness, logits
        self.label = np.ascontiguousarray(label, dtype=F32)    # [N, 6]      mask, x1g, y1g, x2g, y2g, class
        self.fam = list(fam)
        self.hp0 = np.zeros(len(self.fam), dtype=bool) if hp0 is None else np.asarray(hp0, dtype=bool)
        assert len(self.pred) == len(self.label) == len(self.fam) == len(self.hp0)
        for a in (self.pred, self.label, self.hp0):
            a.setflags(write=False)

    @property
    def P(self):
        return self.pred.shape[1]


# ---------------------------------------------------------------------------------------------------------------------------
# CIoU geometry
# ---------------------------------------------------------------------------------------------------------------------------
def _geometry_rows():
    """-> [(family, pred xyxy, label xyxy, anchor or None, scale_pred)], coordinates in 1/64.  anchor: the point the 2^-k scaling holds
    fixed (a border point for the families that live on the border); None: the family is not scaled."""
    rows = []

    def add(fam, p, g=G0, a=(32, 32), sp=True):
        assert p[0] < p[2] and p[1] < p[3] and g[0] < g[2] and g[1] < g[3]
        rows.append((fam, tuple(p), tuple(g), a, sp))

    add("generic", (10, 12, 30, 50))
    add("generic", (24, 30, 60, 44))
    add("identical", G0)
    add("pred_contains_label", (8, 8, 56, 60))
    add("label_contains_pred", (20, 24, 32, 44))
    for k, name in enumerate(("x1", "y1", "x2", "y2")):          # one corner tied; the rest overlapping / inside / outside the label
        for other in ((10, 12, 30, 50), (20, 24, 32, 44), (8, 8, 56, 60)):
            p = list(other)
            p[k] = G0[k]
            add("tie_" + name, p)
    add("tie_two_corners", (16, 12, 40, 50))
    add("tie_two_corners", (10, 20, 30, 52))
    add("touching", (40, 20, 56, 50))        # xk2 == xk1
    add("touching", (4, 20, 16, 50))
    add("touching", (10, 52, 30, 60))        # yk2 == yk1
    add("touching", (40, 52, 56, 60))        # corner to corner
    add("disjoint", (44, 20, 60, 50))
    add("disjoint", (44, 56, 60, 62))
    add("disjoint", (2, 2, 10, 10))
    add("corner_on_border", (0, 12, 30, 50), a=(0, 32))
    add("corner_on_border", (10, 0, 30, 50), a=(32, 0))
    add("corner_on_border", (10, 12, 64, 50), a=(64, 32))
    add("corner_on_border", (10, 12, 30, 64), a=(32, 64))
    add("corner_just_outside", (-1, 12, 30, 50), a=(0, 32))
    add("corner_just_outside", (10, -1, 30, 50), a=(32, 0))
    add("corner_just_outside", (10, 12, 65, 50), a=(64, 32))
    add("corner_just_outside", (10, 12, 30, 65), a=(32, 64))
    add("clamp_meets_label_on_border", (-4, 12, 30, 50), g=(0, 20, 40, 52), a=(0, 32))     # X1 = 0 = x1g
    add("clamp_meets_label_on_border", (10, 12, 70, 50), g=(16, 20, 64, 52), a=(64, 32))   # X2 = 1 = x2g
    add("clamp_meets_label_on_border", (10, -4, 30, 50), g=(16, 0, 40, 52), a=(32, 0))
    add("clamp_meets_label_on_border", (10, 12, 30, 70), g=(16, 20, 40, 64), a=(32, 64))
    add("border_tie_unclamped", (0, 12, 30, 50), g=(0, 20, 40, 52), a=(0, 32))
    add("border_tie_unclamped", (10, 12, 64, 50), g=(16, 20, 64, 52), a=(64, 32))
    add("all_four_clamped", (-8, -8, 72, 72), sp=False)
    add("all_four_clamped", (-8, -8, 72, 72), g=(0, 0, 64, 64), a=None)
    add("pred_beside_image", (-20, 12, -4, 50), a=(0, 32))        # wp == 0, hp > 0
    add("pred_beside_image", (68, 12, 80, 50), a=(64, 32))
    add("square", (10, 12, 30, 50), g=(16, 16, 48, 48))
    add("square", (10, 10, 30, 30))
    add("square", (10, 10, 30, 30), g=(16, 16, 48, 48))          # th == 0
    add("square", (10, 12, 34, 44))                              # same aspect as the label: th == 0
    return rows


def _xyxy_to_cell(p):
    """float64 xyxy -> float32 (cx, cy, w, h) whose float32 corners cx -+ 0.5 w are the xyxy again"""
    p = np.asarray(p, dtype=np.float64)
    c = np.asarray([(p[0] + p[2]) / 2, (p[1] + p[3]) / 2, p[2] - p[0], p[3] - p[1]])
    c32 = c.astype(F32)
    assert np.array_equal(c32.astype(np.float64), c), p
    h = F32(0.5)
    back = np.asarray([c32[0] - h * c32[2], c32[1] - h * c32[3], c32[0] + h * c32[2], c32[1] + h * c32[3]])
    assert back.dtype == F32 and np.array_equal(back.astype(np.float64), p), p
    return c32


def _geometry_cells():
    """-> (family, cxcywh float32 [4], label xyxy float32 [4], hp0)"""
    out = []
    for fam, p, g, a, sp in _geometry_rows():
        for k in range(9 if a is not None else 1):
            f = 2.0 ** -k
            an = np.asarray((a or (0, 0)) * 2, dtype=np.float64)
            ps = (an + (np.asarray(p) - an) * (f if sp else 1.0)) / 64
            gs = (an + (np.asarray(g) - an) * f) / 64
            out.append((f"{fam}/2^-{k}", _xyxy_to_cell(ps), gs.astype(F32), False))
    g = (np.asarray(G0) / 64).astype(F32)
    big = 2.0 ** 33                                              # what t = 80 decodes to, by order of magnitude
    direct = [("size_2^33", (0.5, 0.5, big, 0.25)), ("size_2^33", (0.5, 0.5, 0.25, big)), ("size_2^33", (0.5, 0.5, big, big))]
    for k in (8, 12, 16, 20):
        direct += [("tiny_size", (0.5, 0.5, 2.0 ** -k, 0.25)), ("tiny_size", (0.5, 0.5, 0.25, 2.0 ** -k)), ("tiny_size", (0.5, 0.5, 2.0 ** -k, 2.0 ** -k))]
    # zero-area filter: 0.5 w below half an ulp of cx, so x1 == x2 in float32 only
    direct += [("zero_area", (0.5, 0.5, 2.0 ** -27, 0.25)), ("zero_area", (0.5, 0.5, 0.25, 2.0 ** -27)), ("zero_area", (0.5, 0.5, 2.0 ** -27, 2.0 ** -27)),
               ("zero_area", (0.75, 0.25, 2.0 ** -30, 0.25)), ("zero_area", (0.5, 0.5, 0.0, 0.25))]
    for fam, c in direct:
        out.append((fam, np.asarray(c, dtype=F32), g, False))
    # out of scope, kept as ONE case: clamped to zero HEIGHT with non-zero width (hp == 0): reference autograd gives NaN in x
    out.append(("hp0", _xyxy_to_cell(np.asarray((10, -20, 30, -4)) / 64), g, True))
    return out


def geometry_group(C=2, w=DEFAULT_W):
    cells = _geometry_cells()
    n = len(cells)
    pred = np.zeros((n, 5 + C), dtype=F32)
    label = np.zeros((n, 6), dtype=F32)
    for i, (fam, c, g, hp0) in enumerate(cells):
        pred[i, :4], pred[i, 4] = c, 0.75
        pred[i, 5:] = (np.arange(C) % 3 - 1) * 0.375
        label[i] = (1.0, *g, (i % C))
    return Group(f"geometry_C{C}", pred, label, [c[0] for c in cells], w, [c[3] for c in cells])


# ---------------------------------------------------------------------------------------------------------------------------
# cross-entropy and objectness
# ---------------------------------------------------------------------------------------------------------------------------
_BOX = _xyxy_to_cell(np.asarray((10, 12, 30, 50)) / 64)
_LAB = (np.asarray(G0) / 64).astype(F32)


LSE_FOLD_MAX = F32(16)                                       # head_math.h: the largest |max logit| whose log-sum-exp is folded
_FOLD_UP = float(np.nextafter(LSE_FOLD_MAX, F32(np.inf)))


def ce_group(C, ls):
    rows = []
    ar = np.arange(C, dtype=np.float64)
    even = ar % 2 == 0
    for tgt in sorted({0, C - 1}):
        hot_t = np.zeros(C)
        hot_t[tgt] = 200.0
        hot_o = np.zeros(C)
        hot_o[(tgt + 1) % C] = 200.0
        pats = [("equal_logits", np.full(C, 1.25)), ("one_logit_+200_target", hot_t), ("one_logit_+200_other", hot_o),
                ("logits_+-1e4", np.where(ar % 2 == 0, 1e4, -1e4)), ("logits_-+1e4", np.where(ar % 2 == 0, -1e4, 1e4)),
                ("logits_2^-20_apart", 1.0 + ar * 2.0 ** -20), ("generic_logits", np.sin(1.0 + 2.5 * ar) * 3),
                # either side of the threshold between the two forms of log-softmax, with the largest logit tied over half the classes
                ("max_at_fold", np.where(even, 16.0, 15.0)), ("max_past_fold", np.where(even, _FOLD_UP, 15.0)),
                ("max_at_-fold", np.where(even, -16.0, -17.0)), ("max_past_-fold", np.where(even, -_FOLD_UP, -17.0))]
        for fam, lg in pats:
            for m in (1.0, 0.5):
                rows.append((f"ce_{fam}/m{m:g}", lg, tgt, m))
    pred = np.zeros((len(rows), 5 + C), dtype=F32)
    label = np.zeros((len(rows), 6), dtype=F32)
    for i, (fam, lg, tgt, m) in enumerate(rows):
        pred[i, :4], pred[i, 4], pred[i, 5:] = _BOX, 0.25, lg
        label[i] = (m, *_LAB, tgt)
    return Group(f"ce_C{C}_ls{ls:g}", pred, label, [r[0] for r in rows], (0.5, 5.0, 1.0, ls))


def objectness_group(now):
    rows = [(f"objectness_pred{name}/m{m:g}", po, m) for m in (0.0, 1.0, 0.5)
            for name, po in (("0", 0.0), ("1", 1.0), ("=mask", m), ("_generic", 0.3125))]
    pred = np.zeros((len(rows), 7), dtype=F32)
    label = np.zeros((len(rows), 6), dtype=F32)
    for i, (fam, po, m) in enumerate(rows):
        pred[i, :4], pred[i, 4], pred[i, 5:] = _BOX, po, (0.5, -1.5)
        label[i] = (m, *_LAB, i % 2)
    return Group(f"objectness_now{now:g}", pred, label, [r[0] for r in rows], (now, 5.0, 1.0, 0.01))


@functools.lru_cache(maxsize=None)
def groups():
    gs = [geometry_group(2), geometry_group(1, (0.25, 2.0, 3.0, 0.1))]
    gs += [ce_group(C, ls) for C in (1, 2, 7, 64) for ls in (0.0, 0.01, 0.1)]
    gs += [objectness_group(now) for now in (0.0, 0.25, 0.5, 1.0)]
    return tuple(gs)


# ---------------------------------------------------------------------------------------------------------------------------
# raw-level cases: head outputs for the decode and the fused kernel, one per cell of a [B, P, Sy, Sx] batch
# ---------------------------------------------------------------------------------------------------------------------------
T014 = (0.0, 17.0, -17.0, 88.0, -88.0, 100.0, -100.0)
T80_UP = float(np.nextafter(F32(80), F32(np.inf)))
T23 = (-100.0, -20.0, 0.0, 5.0, 80.0, T80_UP, 90.0)
RAW_C = 3
RAW_LOGITS = ((0.0, 0.0, 0.0), (3.0, -2.0, 1.0), (200.0, 0.0, -200.0), (-1e4, 1e4, 0.0), (1.0, 1.0 + 2.0 ** -20, 1.0 + 2.0 ** -19))
RAW_LABELS = ("mask0", "generic", "full_image", "border_strip")


class RawBatch:
    """B, P, Sy, Sx, w (loss weights), raw [B, P, Sy, Sx], label [B, 6, Sy, Sx] (float32, read-only), fam [B * Sy * Sx] in (b, cell) order, cxs / cys from O.make_grids"""


@functools.lru_cache(maxsize=None)
def raw_batch(B=8):
    Sy, Sx = GRID
    cells = Sy * Sx
    n = B * cells
    P = 5 + RAW_C
    raw = np.zeros((n, P), dtype=F32)
    label = np.zeros((n, 6), dtype=F32)
    fam = []
    g = np.asarray(G0) / 64
    for i in range(n):
        j, r = i % 7, i // 7
        a, b, kind = r % 7, (r // 7) % 7, (r // 49) % 4
        raw[i, :5] = (T014[j], T014[(j + 2) % 7], T23[a], T23[b], T014[(j + 4) % 7])
        raw[i, 5:] = RAW_LOGITS[i % 5]
        m = (0.0, 1.0, 1.0, 0.5)[kind]
        box = (g, g, (0, 0, 1, 1), (0, 20 / 64, 1, 52 / 64) if i % 2 else (16 / 64, 0, 40 / 64, 1))[kind]
        label[i] = (m, *box, i % RAW_C)
        fam.append(f"raw_{RAW_LABELS[kind]}/t2={T23[a]:g},t3={T23[b]:g}")
    out = RawBatch()
    out.B, out.P, out.Sy, out.Sx = B, P, Sy, Sx
    out.raw = np.ascontiguousarray(raw.reshape(B, cells, P).transpose(0, 2, 1).reshape(B, P, Sy, Sx))
    out.label = np.ascontiguousarray(label.reshape(B, cells, 6).transpose(0, 2, 1).reshape(B, 6, Sy, Sx))
    out.fam = fam
    out.cxs, out.cys = O.make_grids(Sx, Sy)
    out.w = DEFAULT_W
    out.raw.setflags(write=False)
    out.label.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# packing a group into a [B, P, Sy, Sx] batch
# ---------------------------------------------------------------------------------------------------------------------------
def pack(group, grid=GRID, min_batch=2, fill=None):
    """-> (pred [B, P, Sy, Sx], label [B, 6, Sy, Sx], case [B * cells] int: the group's case in each slot or -1).  B is a power of two
    >= min_batch (1 / B exact).  Slot i holds case i; with fill="cycle" the remaining slots repeat the cases, otherwise they are
    empty cells (mask 0, objectness 0.5, zero logits)."""
    Sy, Sx = grid
    cells = Sy * Sx
    n = len(group.fam)
    B = min_batch
    while B * cells < n:
        B *= 2
    case = np.full(B * cells, -1, dtype=np.int64)
    case[:n] = np.arange(n)
    if fill == "cycle":
        case = np.arange(B * cells) % n
    pred = np.zeros((B * cells, group.P), dtype=F32)
    pred[:, 4] = 0.5
    label = np.zeros((B * cells, 6), dtype=F32)
    used = case >= 0
    pred[used], label[used] = group.pred[case[used]], group.label[case[used]]
    pred = np.ascontiguousarray(pred.reshape(B, cells, group.P).transpose(0, 2, 1).reshape(B, group.P, Sy, Sx))
    label = np.ascontiguousarray(label.reshape(B, cells, 6).transpose(0, 2, 1).reshape(B, 6, Sy, Sx))
    return pred, label, case


def cells_first(a):
    """[B, P, Sy, Sx] -> [B * Sy * Sx, P]"""
    a = np.asarray(a)
    B, P = a.shape[:2]
    return a.reshape(B, P, -1).transpose(0, 2, 1).reshape(-1, P)


# ---------------------------------------------------------------------------------------------------------------------------
# the references: the oracle's functions per cell, torch autograd
# ---------------------------------------------------------------------------------------------------------------------------
def _valid32(pred32):
    """the reference's zero-area filter, decided in float32 (yogo_loss.py:84-90); pred32 [B, P, Sy, Sx] float32 -> [B * Sy * Sx] bool"""
    assert pred32.dtype == torch.float32
    xyxy = O.box_convert_cxcywh_to_xyxy(pred32[:, :4].permute(0, 2, 3, 1).reshape(-1, 4))
    return torch.logical_and(xyxy[:, 0] != xyxy[:, 2], xyxy[:, 1] != xyxy[:, 3])


def ref_cells(pred, label, w, dtype, inv_batch=1.0, decode=None):
    """pred, label: [B, P, Sy, Sx] / [B, 6, Sy, Sx] float32 arrays.  With decode = (cxs, cys, aw, ah, wm, hm), `pred` is the RAW head
    output and the chain O.decode -> loss is differentiated down to it.
    -> dict(val [3, n] (CIoU, objectness, cross-entropy term of each cell, unweighted), grad [n, P] = d(weighted sum * inv_batch) / d
    input, pred [n, P] (the decoded prediction)), float64 numpy, cells in (b, cell) order."""
    now, iw, cw, ls = w
    x32 = torch.from_numpy(np.array(pred, dtype=F32))
    lab = torch.from_numpy(np.array(label, dtype=F32)).to(dtype)
    x = x32.to(dtype).requires_grad_(True)
    if decode is not None:
        cxs, cys, aw, ah, wm, hm = decode
        p = O.decode(x, cxs.to(dtype), cys.to(dtype), aw, ah, wm, hm)
        with torch.no_grad():
            p32 = O.decode(x32, cxs, cys, aw, ah, wm, hm)
    else:
        p, p32 = x, x32
    assert p.dtype == dtype
    B, P, Sy, Sx = p.shape
    n = B * Sy * Sx
    fp = p[:, :4].permute(0, 2, 3, 1).reshape(n, 4)
    fl = lab[:, 1:5].permute(0, 2, 3, 1).reshape(n, 4)
    m = lab[:, 0].reshape(n)
    sel = torch.logical_and(m.bool(), _valid32(p32))
    xyxy = O.box_convert_cxcywh_to_xyxy(fp[sel])
    ciou = O.complete_box_iou_loss(torch.clamp(xyxy, min=0, max=1), fl[sel], reduction="none")
    iou = torch.zeros(n, dtype=dtype).index_put((sel.nonzero()[:, 0],), ciou)
    cel = F.cross_entropy(p[:, 5:], lab[:, 5].long(), reduction="none", label_smoothing=ls)
    cls = (lab[:, 0] * cel).reshape(n)
    obj = (F.mse_loss(p[:, 4], lab[:, 0], reduction="none") * (lab[:, 0] * (1 - now) + now)).reshape(n)
    total = (obj.sum() + iw * iou.sum() + cw * cls.sum()) * inv_batch
    total.backward()
    return dict(val=torch.stack([iou, obj, cls]).detach().double().numpy(), grad=cells_first(x.grad.double().numpy()),
                pred=cells_first(p.detach().double().numpy()))


def ref_group(group, dtype, inv_batch=1.0):
    """a group's cases as [N, P, 1, 1]"""
    return ref_cells(group.pred[:, :, None, None], group.label[:, :, None, None], group.w, dtype, inv_batch)


def ref_decode(raw, cxs, cys, anchors, inference, gout, dtype):
    """O.decode and its autograd under the upstream gradient gout; [B, P, Sy, Sx] -> (out [n, P], graw [n, P]) float64 numpy"""
    x = torch.from_numpy(np.array(raw, dtype=F32)).to(dtype).requires_grad_(True)
    out = O.decode(x, cxs.to(dtype), cys.to(dtype), *anchors, inference=bool(inference))
    out.backward(torch.from_numpy(np.array(gout, dtype=F32)).to(dtype))
    return cells_first(out.detach().double().numpy()), cells_first(x.grad.double().numpy())


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def scale(r32, r64):
    """[n, k] -> [n]: s = max(max_c |ref32 - ref64|, ulp32(max_c |ref64|)); NaN components (the hp == 0 case) are left out"""
    with np.errstate(invalid="ignore"):
        d = np.nan_to_num(np.abs(r32 - r64), nan=0.0)
        top = np.nan_to_num(np.abs(r64), nan=0.0).max(axis=1)
    return np.maximum(d.max(axis=1), ulp32(top))


def ratios(got, r32, r64):
    """[n, k] -> [n]: max_c |got - ref64| / s.  A NaN or infinity in `got` where the reference is finite counts as infinite."""
    s = scale(r32, r64)
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(got, dtype=np.float64) - r64)
    e = np.where(np.isnan(r64), 0.0, np.where(np.isfinite(e), e, np.inf))
    return e.max(axis=1) / s


def by_family(fam, r):
    """largest ratio per family (the text before '/')"""
    out = {}
    for f, v in zip(fam, r):
        k = f.split("/")[0]
        out[k] = max(out.get(k, 0.0), float(v))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# branch decisions
# ---------------------------------------------------------------------------------------------------------------------------
def live32(pred32, label):
    """the cells that reach the CIoU branches: mask != 0 and the reference's zero-area filter, decided in float32"""
    p = np.asarray(pred32)[:, :4]
    assert p.dtype == F32
    h = F32(0.5)
    return (np.asarray(label)[:, 0] != 0) & (p[:, 0] - h * p[:, 2] != p[:, 0] + h * p[:, 2]) & (p[:, 1] - h * p[:, 3] != p[:, 1] + h * p[:, 3])


def decisions(pred, label, dtype, live):
    """pred [n, >= 4] decoded (cx, cy, w, h), label [n, 6], evaluated in `dtype` -> int8 [n, 13]: the four clamp masks (-1 below 0, 0
    inside or on the border, 1 above 1) and the borders themselves (== 0, == 1 of each corner, folded into one column each), `has`, and
    the sign of each clamped corner against the label's (the eight max / min orderings: max and min of a pair share a comparison)."""
    p = np.asarray(pred)[:, :4].astype(dtype)
    lb = np.asarray(label).astype(dtype)
    h = dtype(0.5)
    c = np.stack([p[:, 0] - h * p[:, 2], p[:, 1] - h * p[:, 3], p[:, 0] + h * p[:, 2], p[:, 1] + h * p[:, 3]], 1)
    assert c.dtype == dtype
    side = np.where(c < 0, -1, np.where(c > 1, 1, 0))
    on = np.where(c == 0, 1, np.where(c == 1, 2, 0))
    X = np.clip(c, dtype(0), dtype(1))
    g = lb[:, 1:5]
    has = (np.minimum(X[:, 3], g[:, 3]) > np.maximum(X[:, 1], g[:, 1])) & (np.minimum(X[:, 2], g[:, 2]) > np.maximum(X[:, 0], g[:, 0]))
    order = np.sign(X - g)
    out = np.concatenate([side, on, has[:, None], order], 1).astype(np.int8)
    # cells that the float32 zero-area filter or an empty mask keeps away from these branches decide nothing
    out[~live] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' statements in numpy float32
# ---------------------------------------------------------------------------------------------------------------------------
VARIANTS = ("tie_weight_1", "tie_weight_0", "exclusive_clamp_mask", "has_ge", "no_eps_D", "no_eps_U", "alpha_gradient_doubled", "dv_swapped",
            "no_half_in_wh", "lt_80", "no_ls_over_C", "class_weight_by_mask_bool", "softmax_bwd_without_dot", "lse_always_folded")


def _sig(x):
    with np.errstate(over="ignore"):
        return F32(1) / (F32(1) + np.exp(-x))


def k_decode(raw, cxs, cys, inv_sx, inv_sy, anchors, inference):
    """decode_fwd_kernel (head_math.h: hm_centre, hm_size, hm_sigmoid, hm_softmax_terms, hm_softmax); raw [n, P], cxs / cys [n] (the cell's grid values)"""
    r = np.asarray(raw, dtype=F32)
    aw, ah, wm, hm = (F32(v) for v in anchors)
    o = np.empty_like(r)
    o[:, 0] = F32(inv_sx) * _sig(r[:, 0]) + cxs.astype(F32)
    o[:, 1] = F32(inv_sy) * _sig(r[:, 1]) + cys.astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        o[:, 2] = aw * np.exp(np.minimum(r[:, 2], F32(80))) * wm
        o[:, 3] = ah * np.exp(np.minimum(r[:, 3], F32(80))) * hm
    o[:, 4] = _sig(r[:, 4])
    if inference:
        with np.errstate(under="ignore"):
            mx = r[:, 5:].max(axis=1)
            sm = np.zeros(len(r), dtype=F32)
            for c in range(5, r.shape[1]):
                sm = sm + np.exp(r[:, c] - mx)
            for c in range(5, r.shape[1]):
                o[:, c] = np.exp(r[:, c] - mx) / sm
    else:
        o[:, 5:] = r[:, 5:]
    assert o.dtype == F32
    return o


def k_decode_bwd(raw, out, gout, inv_sx, inv_sy, inference, var=()):
    """decode_bwd_kernel (head_math.h: hm_centre_bwd, hm_size_bwd, hm_obj_bwd, hm_softmax_bwd_dot, hm_softmax_bwd)"""
    r, o, g = (np.asarray(a, dtype=F32) for a in (raw, out, gout))
    one = F32(1)
    d = np.empty_like(r)
    s0, s1, s4 = _sig(r[:, 0]), _sig(r[:, 1]), o[:, 4]
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        d[:, 0] = g[:, 0] * (F32(inv_sx) * (s0 * (one - s0)))
        d[:, 1] = g[:, 1] * (F32(inv_sy) * (s1 * (one - s1)))
        for k in (2, 3):
            passes = r[:, k] < F32(80) if "lt_80" in var else r[:, k] <= F32(80)
            d[:, k] = np.where(passes, g[:, k] * o[:, k], F32(0))
        d[:, 4] = g[:, 4] * (s4 * (one - s4))
        if inference:
            dot = np.zeros(len(r), dtype=F32)
            if "softmax_bwd_without_dot" not in var:
                for c in range(5, r.shape[1]):
                    dot = dot + g[:, c] * o[:, c]
            for c in range(5, r.shape[1]):
                d[:, c] = o[:, c] * (g[:, c] - dot)
        else:
            d[:, 5:] = g[:, 5:]
    assert d.dtype == F32
    return d


def _logp(x, mx, lsum, var):
    """log_softmax_ of head_math.h: max + log(sum) folded into one constant while |max| <= LSE_FOLD_MAX, the shift first beyond"""
    fold = np.ones_like(mx, dtype=bool) if "lse_always_folded" in var else np.abs(mx) <= LSE_FOLD_MAX
    return np.where(fold, x - (mx + lsum), (x - mx) - lsum)


def k_loss(pred, label, w, inv_batch=1.0, var=()):
    """yogo_loss_kernel (head_math.h: hm_obj_term, hm_ciou_cell, hm_ce_cell, hm_ce_grad), per cell: pred [n, P], label [n, 6] -> (val [3, n], grad [n, P]) float32"""
    pr, lb = np.asarray(pred, dtype=F32), np.asarray(label, dtype=F32)
    now, iw, cw, ls = (F32(v) for v in w)
    ib = F32(inv_batch)
    n, P = pr.shape
    C = P - 5
    one, half, two, zero = F32(1), F32(0.5), F32(2), F32(0)
    tw = F32(1) if "tie_weight_1" in var else F32(0) if "tie_weight_0" in var else half
    m = lb[:, 0]
    grad = np.zeros_like(pr)
    wgt = m * (one - now) + now
    df = pr[:, 4] - m
    l_obj = df * df * wgt
    grad[:, 4] = two * df * wgt * ib

    def dmax_a(a, b):
        return np.where(a > b, one, np.where(a == b, tw, zero))

    def dmin_a(a, b):
        return np.where(a < b, one, np.where(a == b, tw, zero))

    with np.errstate(all="ignore"):
        cx, cy, bw, bh = pr[:, 0], pr[:, 1], pr[:, 2], pr[:, 3]
        x1, y1, x2, y2 = cx - half * bw, cy - half * bh, cx + half * bw, cy + half * bh
        live = (m != zero) & (x1 != x2) & (y1 != y2)
        X1, Y1 = np.minimum(np.maximum(x1, zero), one), np.minimum(np.maximum(y1, zero), one)
        X2, Y2 = np.minimum(np.maximum(x2, zero), one), np.minimum(np.maximum(y2, zero), one)
        if "exclusive_clamp_mask" in var:
            c1, c2, c3, c4 = (((v > zero) & (v < one)).astype(F32) for v in (x1, y1, x2, y2))
        else:
            c1, c2, c3, c4 = (((v >= zero) & (v <= one)).astype(F32) for v in (x1, y1, x2, y2))
        x1g, y1g, x2g, y2g = lb[:, 1], lb[:, 2], lb[:, 3], lb[:, 4]
        eps = F32(1e-7)
        xk1, yk1, xk2, yk2 = np.maximum(X1, x1g), np.maximum(Y1, y1g), np.minimum(X2, x2g), np.minimum(Y2, y2g)
        has = ((yk2 >= yk1) & (xk2 >= xk1)) if "has_ge" in var else ((yk2 > yk1) & (xk2 > xk1))
        iw_, ih = xk2 - xk1, yk2 - yk1
        I = np.where(has, iw_ * ih, zero)
        wp, hp, wg, hg = X2 - X1, Y2 - Y1, x2g - x1g, y2g - y1g
        U = wp * hp + wg * hg - I
        Ue = U if "no_eps_U" in var else U + eps
        iou = I / Ue
        xc1, yc1, xc2, yc2 = np.minimum(X1, x1g), np.minimum(Y1, y1g), np.maximum(X2, x2g), np.maximum(Y2, y2g)
        ex, ey = xc2 - xc1, yc2 - yc1
        D = ex * ex + ey * ey if "no_eps_D" in var else ex * ex + ey * ey + eps
        dxc, dyc = (X2 + X1) / two - (x1g + x2g) / two, (Y2 + Y1) / two - (y1g + y2g) / two
        dist = dxc * dxc + dyc * dyc
        pi = F32(3.14159265358979323846)
        kv = F32(4) / (pi * pi)
        th = np.arctan(wg / hg) - np.arctan(wp / hp)
        v = kv * th * th
        alpha = v / (one - iou + v) if "no_eps_alpha" in var else v / (one - iou + v + eps)
        l_iou = one - iou + dist / D + alpha * v
        dI1 = np.where(has, -ih * dmax_a(X1, x1g), zero)
        dI2 = np.where(has, -iw_ * dmax_a(Y1, y1g), zero)
        dI3 = np.where(has, ih * dmin_a(X2, x2g), zero)
        dI4 = np.where(has, iw_ * dmin_a(Y2, y2g), zero)
        dU1, dU2, dU3, dU4 = -hp - dI1, -wp - dI2, hp - dI3, wp - dI4
        iU2 = one / (Ue * Ue)
        di1, di2 = (dI1 * Ue - I * dU1) * iU2, (dI2 * Ue - I * dU2) * iU2
        di3, di4 = (dI3 * Ue - I * dU3) * iU2, (dI4 * Ue - I * dU4) * iU2
        dD1, dD2 = -two * ex * dmin_a(X1, x1g), -two * ey * dmin_a(Y1, y1g)
        dD3, dD4 = two * ex * dmax_a(X2, x2g), two * ey * dmax_a(Y2, y2g)
        iD2 = one / (D * D)
        dr1, dr2 = (dxc * D - dist * dD1) * iD2, (dyc * D - dist * dD2) * iD2
        dr3, dr4 = (dxc * D - dist * dD3) * iD2, (dyc * D - dist * dD4) * iD2
        den = hp * hp + wp * wp
        dv_dw, dv_dh = -two * kv * th * hp / den, two * kv * th * wp / den
        if "dv_swapped" in var:
            dv_dw, dv_dh = dv_dh, dv_dw
        al = two * alpha if "alpha_gradient_doubled" in var else alpha
        gX1, gY1 = -di1 + dr1 - al * dv_dw, -di2 + dr2 - al * dv_dh
        gX2, gY2 = -di3 + dr3 + al * dv_dw, -di4 + dr4 + al * dv_dh
        sc = iw * ib
        hw = one if "no_half_in_wh" in var else half
        g0 = (gX1 * c1 + gX2 * c3) * sc
        g1 = (gY1 * c2 + gY2 * c4) * sc
        g2 = hw * (gX2 * c3 - gX1 * c1) * sc
        g3 = hw * (gY2 * c4 - gY1 * c2) * sc
    l_iou = np.where(live, l_iou, zero)
    for k, g in enumerate((g0, g1, g2, g3)):
        grad[:, k] = np.where(live, g, zero)
    # cross entropy
    tgt = lb[:, 5].astype(np.int64)
    lg = pr[:, 5:]
    with np.errstate(under="ignore"):
        mx = lg.max(axis=1)
        sm = np.zeros(n, dtype=F32)
        for c in range(C):
            sm = sm + np.exp(lg[:, c] - mx)
        lsum = np.log(sm)
        nll_t, nll_sum = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
        def logp(c):
            return _logp(lg[:, c], mx, lsum, var)

        for c in range(C):
            lp = logp(c)
            nll_sum = nll_sum - lp
            nll_t = np.where(tgt == c, -lp, nll_t)
        lsc = zero if "no_ls_over_C" in var else ls / F32(C)
        l_cls = m * ((one - ls) * nll_t + lsc * nll_sum)
        scl = ((m != zero).astype(F32) if "class_weight_by_mask_bool" in var else m) * cw * ib
        for c in range(C):
            soft = np.exp(logp(c))
            grad[:, 5 + c] = np.where(m != zero, scl * (soft - np.where(tgt == c, one - ls, zero) - lsc), zero)
    l_cls = np.where(m != zero, l_cls, zero)
    val = np.stack([l_iou, l_obj, l_cls])
    assert val.dtype == F32 and grad.dtype == F32
    return val, grad


def k_chain(rb, var=()):
    """decode_loss_bwd_bf16_kernel before its bf16 rounding, on a RawBatch: -> (val [3, n], graw [n, P]) float32"""
    raw, lab = cells_first(rb.raw), cells_first(rb.label)
    cxs = np.tile(rb.cxs.numpy().reshape(-1), rb.B)
    cys = np.tile(rb.cys.numpy().reshape(-1), rb.B)
    inv_sx, inv_sy = F32(1.0 / rb.Sx), F32(1.0 / rb.Sy)
    out = k_decode(raw, cxs, cys, inv_sx, inv_sy, ANCHORS, 0)
    val, gp = k_loss(out, lab, rb.w, 1.0 / rb.B, var)
    return val, k_decode_bwd(raw, out, gp, inv_sx, inv_sy, 0, var), out


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), as float64"""
    return torch.from_numpy(np.asarray(x, dtype=F32).copy()).to(torch.bfloat16).double().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# references computed once and shared by the tests (read-only)
# ---------------------------------------------------------------------------------------------------------------------------
def _freeze(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def group_refs(i):
    """(ref32, ref64) of groups()[i] at inv_batch = 1 (a batch of B = 2^k scales the gradient by exactly 2^-k in both)"""
    g = groups()[i]
    return _freeze(ref_group(g, torch.float32)), _freeze(ref_group(g, torch.float64))


@functools.lru_cache(maxsize=None)
def raw_refs():
    """(ref32, ref64) of the chain O.decode -> loss on raw_batch(), differentiated down to the raw head output, inv_batch = 1 / B"""
    rb = raw_batch()
    dec = (rb.cxs, rb.cys, *ANCHORS)
    return tuple(_freeze(ref_cells(rb.raw, rb.label, rb.w, dt, 1.0 / rb.B, dec)) for dt in (torch.float32, torch.float64))


@functools.lru_cache(maxsize=None)
def decode_refs(inference):
    """upstream gradient gout [B, P, Sy, Sx] float32 and ((out32, graw32), (out64, graw64)) of O.decode on raw_batch()"""
    rb = raw_batch()
    gout = torch.randn(rb.raw.shape, generator=torch.Generator().manual_seed(31 + int(inference))).numpy()
    gout.setflags(write=False)
    return gout, tuple(ref_decode(rb.raw, rb.cxs, rb.cys, ANCHORS, inference, gout, dt) for dt in (torch.float32, torch.float64))
