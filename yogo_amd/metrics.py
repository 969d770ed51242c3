"""``Metrics`` -- the evaluation half behind ``yogo test`` and the end-of-training test (yogo/metrics.py:22-234, called from
yogo/train.py:446-528): prediction <-> label matching (``format_preds_and_labels_v2`` on top of the batched HIP threshold +
NMS kernel), then mAP, confusion matrix, per-class accuracy / precision / recall, ROC curves and calibration error.

The reference delegates the statistics to ``torchmetrics`` (MeanAveragePrecision, MulticlassConfusionMatrix, MulticlassAccuracy,
MulticlassROC(thresholds=500), MulticlassPrecision, MulticlassRecall, MulticlassCalibrationError(n_bins=30)), which is not
installable here; they are restated below from their published definitions (COCO evaluation protocol for mAP) with plain
torch / numpy on the host (the one-box-per-image form ``Metrics`` feeds to mAP is evaluated with array operations over all
images at once: a test split with 10^5 objects takes seconds).  PARITY UNPINNED against a
real torchmetrics (none available); pinned by hand-computed cases in tests/test_metrics.py.

``Metrics(device_matching=True)`` (``yogo test --device-metrics``) runs the matching and the per-batch additions as HIP kernels
(yogo_amd/csrc/match.hip) into accumulators in HBM; ``update`` then reads nothing back (but see ``_DeviceState._reserve_map_rows``) and ``compute`` copies the state once into
the same host objects, so everything after that point is the code below, unchanged.

Quirks of the reference that are kept on purpose:
* ``min_class_confidence_threshold`` defaults to 0.9 (yogo/metrics.py:30) and ``Trainer.test`` / ``yogo test`` run the network
  with ``inference=False``, so the "class confidences" that enter NMS scoring and that threshold are raw logits;
* every matched (prediction, label) pair is handed to mAP as its own one-box "image" (yogo/metrics.py:204-234);
* ``num_classes = len(classes)`` is taken BEFORE the background class is appended (yogo/metrics.py:35-36), while
  ``convert_background_errors(num_classes)`` reuses the LAST real class index for background -- reproduced as is.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from yogo_amd import _hip
from yogo_amd.utils.prediction_formatting import (PredictionLabelMatch, format_preds_and_labels_v2_batched, format_preds_batched,
                                                  gather_device_match, match_rows_to_labels_device, raise_for_match_status)


# ---------------------------------------------------------------------------------------------------------------------
# COCO mean average precision (the protocol torchmetrics.detection.MeanAveragePrecision implements)
# ---------------------------------------------------------------------------------------------------------------------
_IOU_THRS = np.linspace(0.5, 0.95, 10)
_REC_THRS = np.linspace(0.0, 1.0, 101)
_MAX_DETS = (1, 10, 100)
_AREAS = {"all": (0.0, 1e10), "small": (0.0, 32.0 ** 2), "medium": (32.0 ** 2, 96.0 ** 2), "large": (96.0 ** 2, 1e10)}


def _box_iou_np(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a[:, None] + area_b[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union > 0, inter / union, 0.0)


class _PairBlock(tuple):
    """K one-detection / one-ground-truth images as arrays (det boxes [K,4], scores [K], labels [K], gt boxes [K,4], labels [K]):
    one entry of ``MeanAveragePrecision._images`` standing for K images, in the order they were handed in"""


class MeanAveragePrecision:
    """COCO mAP over lists of per-image dicts: preds {boxes [n,4] xyxy, scores [n], labels [n]}, targets {boxes, labels}."""

    def __init__(self, box_format: str = "xyxy") -> None:
        if box_format != "xyxy":
            raise ValueError("only box_format='xyxy' is supported")
        self.reset()

    def reset(self) -> None:
        self._images: List[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]] = []

    def update(self, preds: List[Dict[str, torch.Tensor]], targets: List[Dict[str, torch.Tensor]]) -> None:
        if len(preds) != len(targets):
            raise ValueError("preds and targets must have the same length")
        for p, t in zip(preds, targets):
            self._images.append((
                p["boxes"].detach().cpu().double().numpy().reshape(-1, 4), p["scores"].detach().cpu().double().numpy().reshape(-1),
                p["labels"].detach().cpu().long().numpy().reshape(-1),
                t["boxes"].detach().cpu().double().numpy().reshape(-1, 4), t["labels"].detach().cpu().long().numpy().reshape(-1)))

    def update_pairs(self, det_boxes, det_scores, det_labels, gt_boxes, gt_labels) -> None:
        """K images of exactly one detection and one ground truth each, as [K, ...] arrays (tensors or numpy) -- the same state as
        ``update`` on the K one-box dicts ``Metrics._format_for_mAP`` makes, without a Python object per row"""
        def arr(x, dtype, shape):
            x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
            return np.ascontiguousarray(x.astype(dtype, copy=False)).reshape(shape)

        db, gb = arr(det_boxes, np.float64, (-1, 4)), arr(gt_boxes, np.float64, (-1, 4))
        ds, dl, gl = arr(det_scores, np.float64, (-1,)), arr(det_labels, np.int64, (-1,)), arr(gt_labels, np.int64, (-1,))
        if not (len(db) == len(ds) == len(dl) == len(gb) == len(gl)):
            raise ValueError("update_pairs: the five arrays must have the same number of rows")
        if len(db):
            self._images.append(_PairBlock((db, ds, dl, gb, gl)))

    def _per_image(self):
        """every entry as one (boxes, scores, labels, gt boxes, gt labels) image -- the general path's view"""
        for im in self._images:
            if isinstance(im, _PairBlock):
                for k in range(len(im[1])):
                    yield (im[0][k:k + 1], im[1][k:k + 1], im[2][k:k + 1], im[3][k:k + 1], im[4][k:k + 1])
            else:
                yield im

    def _evaluate_image(self, img, cls: int, area: Tuple[float, float], max_det: int):
        db, ds, dl, gb, gl = img
        dsel, gsel = dl == cls, gl == cls
        if not dsel.any() and not gsel.any():
            return None
        db, ds, gb = db[dsel], ds[dsel], gb[gsel]
        order = np.argsort(-ds, kind="mergesort")[:max_det]
        db, ds = db[order], ds[order]
        g_area = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
        g_ign = (g_area < area[0]) | (g_area > area[1])
        gorder = np.argsort(g_ign, kind="mergesort")          # non-ignored ground truth first
        gb, g_ign = gb[gorder], g_ign[gorder]
        ious = _box_iou_np(db, gb) if len(db) and len(gb) else np.zeros((len(db), len(gb)))
        T, D, G = len(_IOU_THRS), len(db), len(gb)
        dm = np.zeros((T, D), dtype=bool)
        d_ign = np.zeros((T, D), dtype=bool)
        gm = np.zeros((T, G), dtype=bool)
        for ti, thr in enumerate(_IOU_THRS):
            for d in range(D):
                best, m = min(thr, 1 - 1e-10), -1
                for g in range(G):
                    if gm[ti, g]:
                        continue
                    if m > -1 and not g_ign[m] and g_ign[g]:
                        break                                  # a non-ignored match beats every ignored one
                    if ious[d, g] < best:
                        continue
                    best, m = ious[d, g], g
                if m > -1:
                    dm[ti, d], d_ign[ti, d], gm[ti, m] = True, g_ign[m], True
        d_area = (db[:, 2] - db[:, 0]) * (db[:, 3] - db[:, 1])
        out_of_range = (d_area < area[0]) | (d_area > area[1])
        d_ign = d_ign | (~dm & out_of_range[None, :])
        return ds, dm, d_ign, int((~g_ign).sum())

    @staticmethod
    def _accumulate(precision, recall, ki, ai, mis, scores, dm, dig, npig) -> None:
        """precision at the 101 recall points and the final recall of one (class, area) cell, written for every max-det index in mis"""
        T, R = len(_IOU_THRS), len(_REC_THRS)
        order = np.argsort(-scores, kind="mergesort")
        dm, dig = dm[:, order], dig[:, order]
        tps = np.cumsum(dm & ~dig, axis=1, dtype=np.float64)
        fps = np.cumsum(~dm & ~dig, axis=1, dtype=np.float64)
        nd = tps.shape[1]
        for ti in range(T):
            tp, fp = tps[ti], fps[ti]
            rc = tp / npig
            pr = tp / (tp + fp + np.spacing(1))
            pr = np.maximum.accumulate(pr[::-1])[::-1]           # precision envelope
            inds = np.searchsorted(rc, _REC_THRS, side="left")
            q = np.zeros(R)
            ok = inds < nd
            q[ok] = pr[inds[ok]]
            for mi in mis:
                recall[ti, ki, ai, mi] = rc[-1] if nd else 0
                precision[ti, :, ki, ai, mi] = q

    def _compute_single_box_images(self, classes, precision, recall) -> None:
        """the case ``Metrics`` produces (yogo/metrics.py:204-234: every matched pair is its own image with at most one detection
        and one ground truth): the per-image greedy matching collapses to one IoU per image, so a (class, area) cell is a few
        array operations over all images, and the three max-det settings (>= 1) give the same cell."""
        N = sum(len(im[1]) if isinstance(im, _PairBlock) else 1 for im in self._images)
        d_has, g_has = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
        d_box, g_box = np.zeros((N, 4)), np.zeros((N, 4))
        d_score, d_lab, g_lab = np.zeros(N), np.full(N, -1, dtype=np.int64), np.full(N, -1, dtype=np.int64)
        i = 0
        for im in self._images:
            db, ds, dl, gb, gl = im
            if isinstance(im, _PairBlock):               # K rows at once
                k = len(ds)
                d_has[i:i + k], g_has[i:i + k] = True, True
                d_box[i:i + k], d_score[i:i + k], d_lab[i:i + k], g_box[i:i + k], g_lab[i:i + k] = db, ds, dl, gb, gl
                i += k
                continue
            d_has[i], g_has[i] = len(ds) == 1, len(gl) == 1
            if d_has[i]:
                d_box[i], d_score[i], d_lab[i] = db[0], ds[0], dl[0]
            if g_has[i]:
                g_box[i], g_lab[i] = gb[0], gl[0]
            i += 1
        d_area = (d_box[:, 2] - d_box[:, 0]) * (d_box[:, 3] - d_box[:, 1])
        g_area = (g_box[:, 2] - g_box[:, 0]) * (g_box[:, 3] - g_box[:, 1])
        lt, rb = np.maximum(d_box[:, :2], g_box[:, :2]), np.minimum(d_box[:, 2:], g_box[:, 2:])
        wh = np.clip(rb - lt, 0, None)
        inter = wh[:, 0] * wh[:, 1]
        union = d_area + g_area - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = np.where(union > 0, inter / union, 0.0)
        thr = np.minimum(_IOU_THRS, 1 - 1e-10)[:, None]
        for ki, cls in enumerate(classes):
            dsel, gsel = d_has & (d_lab == cls), g_has & (g_lab == cls)
            for ai, area in enumerate(_AREAS.values()):
                g_ign = gsel & ((g_area < area[0]) | (g_area > area[1]))
                npig = int((gsel & ~g_ign).sum())
                if npig == 0:
                    continue
                dm = (dsel & gsel)[None, :] & (iou[None, :] >= thr)
                dig = (dm & g_ign[None, :]) | (~dm & ((d_area < area[0]) | (d_area > area[1]))[None, :])
                self._accumulate(precision, recall, ki, ai, range(len(_MAX_DETS)), d_score[dsel], dm[:, dsel], dig[:, dsel], npig)

    def compute(self, _general: bool = False) -> Dict[str, torch.Tensor]:
        classes = sorted({int(c) for im in self._images for c in np.unique(np.concatenate((im[2], im[4])))})
        T, R, K, A, M = len(_IOU_THRS), len(_REC_THRS), len(classes), len(_AREAS), len(_MAX_DETS)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        single = not _general and all(isinstance(im, _PairBlock) or (len(im[1]) <= 1 and len(im[4]) <= 1) for im in self._images)
        if single:
            self._compute_single_box_images(classes, precision, recall)
        for ki, cls in enumerate([] if single else classes):
            imgs = [im for im in self._per_image() if (im[2] == cls).any() or (im[4] == cls).any()]
            for ai, area in enumerate(_AREAS.values()):
                for mi, max_det in enumerate(_MAX_DETS):
                    ev = [e for e in (self._evaluate_image(im, cls, area, max_det) for im in imgs) if e is not None]
                    if not ev:
                        continue
                    npig = sum(e[3] for e in ev)
                    if npig == 0:
                        continue
                    self._accumulate(precision, recall, ki, ai, (mi,), np.concatenate([e[0] for e in ev]),
                                     np.concatenate([e[1] for e in ev], axis=1), np.concatenate([e[2] for e in ev], axis=1), npig)

        def mean_valid(x):
            x = x[x > -1]
            return torch.tensor(float(x.mean()) if x.size else -1.0)

        areas = list(_AREAS)
        out = {
            "map": mean_valid(precision[:, :, :, 0, 2]),
            "map_50": mean_valid(precision[0, :, :, 0, 2]),
            "map_75": mean_valid(precision[5, :, :, 0, 2]),
            "map_small": mean_valid(precision[:, :, :, areas.index("small"), 2]),
            "map_medium": mean_valid(precision[:, :, :, areas.index("medium"), 2]),
            "map_large": mean_valid(precision[:, :, :, areas.index("large"), 2]),
            "mar_1": mean_valid(recall[:, :, 0, 0]),
            "mar_10": mean_valid(recall[:, :, 0, 1]),
            "mar_100": mean_valid(recall[:, :, 0, 2]),
            "mar_small": mean_valid(recall[:, :, areas.index("small"), 2]),
            "mar_medium": mean_valid(recall[:, :, areas.index("medium"), 2]),
            "mar_large": mean_valid(recall[:, :, areas.index("large"), 2]),
            "map_per_class": torch.tensor(-1.0),
            "mar_100_per_class": torch.tensor(-1.0),
            "classes": torch.tensor(classes, dtype=torch.int32),
        }
        return out


# ---------------------------------------------------------------------------------------------------------------------
# classification statistics over the matched rows
# ---------------------------------------------------------------------------------------------------------------------
def _as_probabilities(scores: torch.Tensor) -> torch.Tensor:
    """torchmetrics' normalisation for curve / calibration metrics: softmax unless the scores already lie in [0, 1]"""
    if scores.numel() and not bool(((scores >= 0) & (scores <= 1)).all()):
        return scores.softmax(1)
    return scores


def _safe_div(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.where(b != 0, a / torch.where(b != 0, b, torch.ones_like(b)), torch.zeros_like(a))


class _ClassStats:
    """confusion matrix (rows = true class, columns = predicted class), binned one-vs-rest ROC states, calibration bins"""

    def __init__(self, num_classes: int, roc_thresholds: int = 500, n_bins: int = 30) -> None:
        self.C = num_classes
        self.thresholds = torch.linspace(0, 1, roc_thresholds, dtype=torch.float64)
        self.n_bins = n_bins
        self.reset()

    def reset(self) -> None:
        self.confmat = torch.zeros(self.C, self.C, dtype=torch.long)
        self.roc_tp = torch.zeros(len(self.thresholds), self.C, dtype=torch.long)   # predicted positive & is class
        self.roc_fp = torch.zeros(len(self.thresholds), self.C, dtype=torch.long)
        self.pos = torch.zeros(self.C, dtype=torch.long)
        self.n = 0
        self.bin_count = torch.zeros(self.n_bins, dtype=torch.float64)
        self.bin_conf = torch.zeros(self.n_bins, dtype=torch.float64)
        self.bin_acc = torch.zeros(self.n_bins, dtype=torch.float64)

    def update(self, scores: torch.Tensor, target: torch.Tensor) -> None:
        scores = scores.detach().cpu().double().reshape(-1, scores.shape[-1])
        target = target.detach().cpu().long().reshape(-1)
        if scores.shape[0] == 0:
            return
        pred = scores.argmax(1)
        valid = (target >= 0) & (target < self.C) & (pred < self.C)
        idx = target[valid] * self.C + pred[valid]
        self.confmat += torch.bincount(idx, minlength=self.C * self.C).view(self.C, self.C)
        prob = _as_probabilities(scores)[:, : self.C]
        onehot = torch.nn.functional.one_hot(target.clamp(0, self.C - 1), self.C).bool() & ((target >= 0) & (target < self.C))[:, None]
        above = prob[None, :, :] >= self.thresholds[:, None, None]                  # [T, N, C]
        self.roc_tp += (above & onehot[None]).sum(1)
        self.roc_fp += (above & ~onehot[None]).sum(1)
        self.pos += onehot.sum(0)
        self.n += scores.shape[0]
        conf, arg = prob.max(1)
        acc = (arg == target).double()
        edges = torch.linspace(0, 1, self.n_bins + 1, dtype=torch.float64)
        b = (torch.bucketize(conf, edges, right=True) - 1).clamp(0, self.n_bins - 1)
        self.bin_count += torch.bincount(b, minlength=self.n_bins).double()
        self.bin_conf += torch.bincount(b, weights=conf, minlength=self.n_bins)
        self.bin_acc += torch.bincount(b, weights=acc, minlength=self.n_bins)

    def compute(self) -> Dict[str, Any]:
        cm = self.confmat.double()
        tp = cm.diag()
        support, predicted = cm.sum(1), cm.sum(0)
        recall = _safe_div(tp, support)
        precision = _safe_div(tp, predicted)
        neg = (self.n - self.pos).double()
        tpr = _safe_div(self.roc_tp.double(), self.pos.double()[None, :].expand_as(self.roc_tp)).flip(0).T   # [C, T], thresholds descending
        fpr = _safe_div(self.roc_fp.double(), neg[None, :].expand_as(self.roc_fp)).flip(0).T
        cnt = self.bin_count
        prop = cnt / cnt.sum() if float(cnt.sum()) > 0 else cnt
        ece = float((_safe_div(self.bin_acc, cnt) - _safe_div(self.bin_conf, cnt)).abs().mul(prop).sum())
        return {
            "MulticlassAccuracy": recall.float(),          # torchmetrics' per-class accuracy (average=None) = per-class recall
            "MulticlassPrecision": precision.float(),
            "MulticlassRecall": recall.float(),
            "MulticlassROC": (fpr.float(), tpr.float(), self.thresholds.flip(0).float()),
            "MulticlassCalibrationError": torch.tensor(ece),
        }


class _DeviceState:
    """The accumulators of ``Metrics(device_matching=True)`` in HBM (include/yogo_hip.h: yogo_metrics_accumulate): the integer state
    (confusion matrix, positives, counts by class, calibration bins, the ROC histogram over k = #{thresholds <= p}), the fp64
    confidence sums, and the rows mAP needs per matched pair.  The device is read back by ``map_rows_host`` /
    ``Metrics._read_device_state`` (from ``compute``) and, when its bound overflows, by the capacity check of the mAP buffer."""

    MAP_ROW = 11

    def __init__(self, device: torch.device, C: int, thresholds: torch.Tensor, n_bins: int, include_mAP: bool) -> None:
        self.device, self.C, self.T, self.nb = device, C, int(thresholds.numel()), n_bins
        layout = (ctypes.c_longlong * 12)()
        _hip.call("yogo_metrics_state_layout", C, self.T, n_bins, ctypes.addressof(layout))   # the library owns the layout
        (_, self.off_pos, self.off_n, self.off_missed, self.off_extra, self.off_total, self.off_bin_count, self.off_bin_acc, self.off_hist,
         self.off_map_count, self.off_status, words) = (int(v) for v in layout)
        self.acc = torch.zeros(words, dtype=torch.int64, device=device)
        self.bin_conf = torch.zeros(n_bins, dtype=torch.float64, device=device)
        # the very doubles the host statistics compare against (never regenerated on the device)
        self.thresholds = thresholds.to(device=device, dtype=torch.float64).contiguous()
        self.edges = torch.linspace(0, 1, n_bins + 1, dtype=torch.float64).to(device)
        self.include_mAP = include_mAP
        self.map_rows: Optional[torch.Tensor] = None
        self._rows_bound = 0          # upper bound of the mAP rows appended so far
        self._pending: List[Tuple[torch.cuda.Event, torch.Tensor, int]] = []   # per update: (event after it, total rows after it, its bound)

    def _reserve_map_rows(self, need: int) -> None:
        """room for `need` more rows.  The host knows only a bound per update (an image has at most min(labels, rows) pairs, and both
        counts live on the device), so the exact total of the latest FINISHED update, copied asynchronously after each one, replaces the
        bounds up to it.  Only when the bound still does not fit is the counter itself read -- the one place where ``update`` may
        wait, and only for metrics launches already queued; the buffer then grows if the exact count needs it.  The first buffer
        holds two updates' bounds: a caller that synchronises once per batch (``Trainer.test`` reads the loss) never waits here."""
        done = None
        while self._pending and self._pending[0][0].query():
            done = self._pending.pop(0)
        if done is not None:          # its count is the total after that update; the later ones are still bounds
            self._rows_bound = int(done[1]) + sum(bound for _, _, bound in self._pending)
        if self.map_rows is None:
            self.map_rows = torch.empty(max(2 * need, 1), self.MAP_ROW, dtype=torch.float32, device=self.device)
        if self._rows_bound + need > self.map_rows.shape[0]:
            exact = int(self.acc[self.off_map_count])
            self._pending.clear()
            self._rows_bound = exact
            if exact + need > self.map_rows.shape[0]:
                grown = torch.empty(max(2 * self.map_rows.shape[0], exact + 2 * need), self.MAP_ROW, dtype=torch.float32, device=self.device)
                grown[:exact] = self.map_rows[:exact]
                self.map_rows = grown
        self._rows_bound += need

    def accumulate(self, dm) -> None:
        B, cap, P = dm.rows.shape
        with torch.cuda.device(self.device):
            if self.include_mAP:
                self._reserve_map_rows(B * cap)
            partial = torch.empty(B, self.nb, dtype=torch.float64, device=self.device)
            _hip.call("yogo_metrics_accumulate", *dm.tail, self.thresholds, self.T, self.edges, self.nb, self.acc, self.bin_conf, partial,
                      self.map_rows if self.include_mAP else None, self.map_rows.shape[0] if self.include_mAP else 0, B, P, cap,
                      _hip.stream_ptr())
            if self.include_mAP:
                count = torch.empty(1, dtype=torch.int64).pin_memory()
                count.copy_(self.acc[self.off_map_count: self.off_map_count + 1], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._pending.append((ev, count, B * cap))

    def map_rows_host(self, count: int) -> torch.Tensor:
        if self.map_rows is None or count == 0:
            return torch.zeros(0, self.MAP_ROW)
        if count > self.map_rows.shape[0]:
            raise RuntimeError(f"yogo_amd: {count} matched pairs were counted but the mAP buffer holds {self.map_rows.shape[0]} rows")
        return self.map_rows[:count].cpu()

    def reset(self) -> None:
        """what ``Metrics.reset`` resets on the host: the class statistics and mAP, not the missed / extra / total counters; and the
        two status counts, so that an object is usable again after a batch that ``compute`` refused"""
        self.acc[: self.off_missed].zero_()
        self.acc[self.off_bin_count:].zero_()
        self.bin_conf.zero_()
        self._pending.clear()
        self._rows_bound = 0


class Metrics:
    """yogo/metrics.py:22-234 -- same constructor, ``update`` / ``compute`` / ``reset`` / ``forward`` and return tuple."""

    @torch.no_grad()
    def __init__(
        self,
        classes: List[str],
        device: str = "cpu",
        sync_on_compute: bool = False,
        min_class_confidence_threshold: float = 0.9,
        include_mAP: bool = True,
        include_background: bool = True,
        device_matching: bool = False,
    ):
        self.device_matching = bool(device_matching)   # match and accumulate on the MI355X (yogo_amd/csrc/match.hip); same results
        self._dev: Optional[_DeviceState] = None
        self.device = device
        self.classes = classes + (["background"] if include_background else [])
        self.num_classes = len(classes)
        self.min_class_confidence_threshold = min_class_confidence_threshold
        self.include_mAP = include_mAP
        self.include_background = include_background
        self.sync_on_compute = sync_on_compute          # (the reference never synchronises either: train.py:465-471)
        if include_mAP:
            self.mAP = MeanAveragePrecision(box_format="xyxy")
        self._stats = _ClassStats(self.num_classes)
        self.num_obj_missed_by_class = torch.zeros(self.num_classes, dtype=torch.long)
        self.num_obj_extra_by_class = torch.zeros(self.num_classes, dtype=torch.long)
        self.total_num_true_objects = torch.zeros(1, dtype=torch.long)

    @torch.no_grad()
    def update(self, preds: torch.Tensor, labels: torch.Tensor, use_IoU: bool = True) -> None:
        if self.device_matching:
            plm = self._update_device(preds, labels)
            if plm is None:
                return                                   # accumulated on the device; read out by compute()
        else:
            # one batched threshold + NMS launch for the whole batch, then the per-image Hungarian matching on the host
            matches = format_preds_and_labels_v2_batched(preds.detach(), labels.detach(),
                                                         min_class_confidence_threshold=self.min_class_confidence_threshold)
            plm = PredictionLabelMatch.concat(matches)

        def count_classes(cls: torch.Tensor) -> torch.Tensor:
            values, counts = cls.unique(return_counts=True)
            out = torch.zeros(self.num_classes, dtype=torch.long)
            out[values.long()] = counts
            return out

        if plm.missed_labels is not None:
            self.num_obj_missed_by_class += count_classes(plm.missed_labels[:, 5].cpu())
        if plm.extra_predictions is not None:
            self.num_obj_extra_by_class += count_classes(plm.extra_predictions[:, 5:].argmax(dim=1).cpu())
        self.total_num_true_objects += plm.labels.shape[0]
        if self.include_background:
            plm = plm.convert_background_errors(self.num_classes)
        fps, fls = plm.preds, plm.labels
        if self.include_mAP:
            self.mAP.update(*self._format_for_mAP(fps, fls))
        self._stats.update(fps[:, 5:], fls[:, 5:].squeeze(-1))

    def _update_device(self, preds, labels) -> Optional[PredictionLabelMatch]:
        """threshold + NMS launch, match launch, then either the accumulate launch (nothing is read back; returns None) or, with
        ``include_background``, the gathered match on the host for the unchanged background conversion and host statistics"""
        if isinstance(preds, torch.Tensor):
            preds = preds.detach()
            _hip.require_cuda(preds, "preds")
        rows, _, counts = format_preds_batched(preds, 0.5, 0.5, "xyxy", self.min_class_confidence_threshold)
        dm = match_rows_to_labels_device(rows, counts, labels.detach().to(rows.device))
        if self.include_background:
            plm = gather_device_match(dm)
            return PredictionLabelMatch(plm.preds.cpu(), plm.labels.cpu(), plm.missed_labels.cpu(), plm.extra_predictions.cpu())
        if rows.shape[2] - 5 != self.num_classes:
            raise ValueError(f"predictions carry {rows.shape[2] - 5} class scores, the metrics were built for {self.num_classes} classes")
        if self._dev is None:
            self._dev = _DeviceState(rows.device, self.num_classes, self._stats.thresholds, self._stats.n_bins, self.include_mAP)
        if rows.shape[0]:
            self._dev.accumulate(dm)
        return None

    def _read_device_state(self) -> None:
        """the accumulators of the device path into the host objects ``compute`` reads (one copy; idempotent).  Raises scipy's
        ``ValueError`` if an image of any update since the last ``reset`` had an invalid or infeasible cost matrix.  Unlike the host
        path, where the offending ``update`` raises before it adds anything, the OTHER images of such a batch have been added by then:
        the sums are partial and the object is to be ``reset``."""
        d = self._dev
        acc = d.acc.cpu()
        C, nb = self.num_classes, self._stats.n_bins
        raise_for_match_status(int(acc[d.off_status]), int(acc[d.off_status + 1]))
        st = self._stats
        st.confmat = acc[: C * C].view(C, C).clone()
        st.pos = acc[d.off_pos: d.off_pos + C].clone()
        st.n = int(acc[d.off_n])
        st.bin_count = acc[d.off_bin_count: d.off_bin_count + nb].double()
        st.bin_acc = acc[d.off_bin_acc: d.off_bin_acc + nb].double()
        st.bin_conf = d.bin_conf.cpu()
        hist = acc[d.off_hist: d.off_map_count].view(-1, C, 2)            # [T + 1, C, is-target], k = #{thresholds <= p}
        above = hist.flip(0).cumsum(0).flip(0)[1:]                        # [T, C, 2]: #{p >= threshold t} = sum over k > t
        st.roc_tp, st.roc_fp = above[:, :, 1].contiguous(), above[:, :, 0].contiguous()
        self.num_obj_missed_by_class = acc[d.off_missed: d.off_missed + C].clone()
        self.num_obj_extra_by_class = acc[d.off_extra: d.off_extra + C].clone()
        self.total_num_true_objects = acc[d.off_total: d.off_total + 1].clone()
        if self.include_mAP:
            rows = d.map_rows_host(int(acc[d.off_map_count]))
            self.mAP.reset()
            self.mAP.update_pairs(rows[:, :4], rows[:, 4], rows[:, 5], rows[:, 6:10], rows[:, 10])

    @torch.no_grad()
    def compute(self) -> Tuple[Any, ...]:
        if self._dev is not None:
            self._read_device_state()
        pr = self._stats.compute()
        mAP_metrics = self.mAP.compute() if self.include_mAP else {"map": torch.tensor(0.0)}
        return (
            mAP_metrics,
            self._stats.confmat.clone(),
            pr["MulticlassAccuracy"],
            pr["MulticlassROC"],
            pr["MulticlassPrecision"],
            pr["MulticlassRecall"],
            pr["MulticlassCalibrationError"].item(),
            self.num_obj_missed_by_class.cpu(),
            self.num_obj_extra_by_class.cpu(),
            self.total_num_true_objects.cpu(),
        )

    @torch.no_grad()
    def get_wandb_confusion_matrix(self, confusion_metrics):
        """the reference turns the matrix into a wandb table (yogo/utils/utils.py:50-129); wandb is optional here, so the
        rows (true class, predicted class, count) are returned as plain data"""
        names = self.classes
        return [[names[i] if i < len(names) else str(i), names[j] if j < len(names) else str(j), int(confusion_metrics[i, j])]
                for i in range(confusion_metrics.shape[0]) for j in range(confusion_metrics.shape[1])]

    def reset(self) -> None:
        if self.include_mAP:
            self.mAP.reset()
        self._stats.reset()
        if self._dev is not None:
            self._dev.reset()

    @torch.no_grad()
    def forward(self, preds, labels):
        self.update(preds, labels)
        res = self.compute()
        self.reset()
        return res

    def _format_for_mAP(self, preds: torch.Tensor, labels: torch.Tensor):
        """every matched pair becomes its own one-box image (yogo/metrics.py:204-234)"""
        fp, fl = [], []
        for p, l in zip(preds, labels):
            fp.append({"boxes": p[:4].reshape(1, 4), "scores": p[4].reshape(1), "labels": p[5:].argmax().reshape(1)})
            fl.append({"boxes": l[1:5].reshape(1, 4), "labels": l[5].reshape(1).long()})
        return fp, fl
