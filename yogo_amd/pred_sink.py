"""``PredictionSink`` -- the output stage of ``predict(..., device_outputs=True)`` / ``yogo infer --device-outputs``.

The default path of ``predict`` copies the padded ``rows [B, cap, 5+C]`` of every batch to the host (``save_predictions``,
``format_to_numpy_batched``) and counts classes per image from Python (``get_prediction_class_counts``): one synchronisation, or B of
them, per batch.  A sink instead hands ``rows`` / ``counts`` of ``format_preds_batched`` to ``yogo_pred_sink_append``
(yogo_amd/csrc/pred_sink.hip), which compacts the kept rows into an arena in HBM (as ``.npy`` records or as they are), appends the
per-image counts and adds to a class histogram; the host reads the arena once per ``drain()`` -- at the end of a run, or when
``should_flush()`` says that ``flush_rows`` records have piled up.  What comes out is bit for bit what the host path computes.

The text of ``--save-preds`` is written on the device as well: ``drain_text()`` hands the arena of a "rows" sink to
``yogo_pred_text_format`` (yogo_amd/csrc/pred_text.hip), which prints every row as ``prediction_rows_to_text`` does -- shortest
round-trip decimals, byte for byte what Python's ``repr`` gives -- and the host reads the finished bytes of all images and their
offsets.  Only the file writes stay on the host (``split_records`` gives ``drain()``'s callers their per-image views).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from yogo_amd import _hip

MODE_NPY = 0    # records of 8 + C floats: the columns of format_to_numpy
MODE_ROWS = 1   # records of 5 + C floats: the kept rows
_MODES = {"npy": MODE_NPY, "rows": MODE_ROWS, MODE_NPY: MODE_NPY, MODE_ROWS: MODE_ROWS}

# Drain once this many records are known to be in the arena.  A record is at most 4 * (8 + C) bytes: 2^21 records of C = 7 are
# 126 MB, a few minutes of production frames (~96 records each).  The arena itself is larger than that by the BOUNDS of the appends
# in flight (B * cap records each, see ``_reserve``): at the production geometry and B = 256 two of them are 6.4 M records, so a
# sink stays under ~400 MB there and under ~100 MB at the CLI's B = 64.
DEFAULT_FLUSH_ROWS = 1 << 21


def state_layout(num_classes: int) -> Tuple[int, int, int, int, int, int]:
    """(records, images, dropped records, dropped image entries, class_counts, words): where each lives in the int64 state block.
    The library owns the layout; the query runs on the host."""
    layout = (ctypes.c_longlong * 6)()
    _hip.call("yogo_pred_sink_state_layout", int(num_classes), ctypes.addressof(layout))
    return tuple(int(v) for v in layout)   # type: ignore[return-value]


def split_records(records: np.ndarray, per_image_counts) -> List[np.ndarray]:
    """the per-image views of drained records [N, reclen], in order; an image without rows gets a [0, reclen] view"""
    counts = np.asarray(per_image_counts, dtype=np.int64).reshape(-1)
    if counts.size and int(counts.min()) < 0:
        raise ValueError("split_records: negative per-image count")
    ends = np.cumsum(counts)
    if (int(ends[-1]) if counts.size else 0) != records.shape[0]:
        raise ValueError(f"split_records: the counts sum to {int(ends[-1]) if counts.size else 0}, there are {records.shape[0]} records")
    return [records[e - c: e] for c, e in zip(counts.tolist(), ends.tolist())]


def npy_columns(chunks, num_classes: int) -> np.ndarray:
    """the ``(8 + C) x N`` array ``predict`` saves, from drained npy-mode chunks ``[(records, per_image_counts), ...]``: what
    ``np.hstack`` of the default path's per-image ``format_to_numpy`` arrays gives, memory order included (``np.save`` records it, and
    numpy derives it from the strides of the pieces: an image's columns are its records transposed, an image without rows is a
    fresh ``(8 + C, 0)`` array, exactly as there), so the file is the same byte for byte"""
    parts = [r.T if len(r) else np.zeros((records.shape[1], 0), dtype=np.float32)
             for records, per_image in chunks for r in split_records(records, per_image)]
    return np.hstack(parts) if parts else np.zeros((8 + num_classes, 0), dtype=np.float32)


class PredictionSink:
    """Kept rows of many batches, compacted and counted in HBM.  ``mode`` "npy" (needs ``img_hw``) or "rows"; ``append`` and
    ``add_counts`` launch and return, ``drain`` (or ``drain_text``) is the one read."""

    def __init__(self, device: Union[str, torch.device], num_classes: int, mode: Union[str, int], img_hw: Optional[Tuple[int, int]] = None,
                 flush_rows: int = DEFAULT_FLUSH_ROWS) -> None:
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"yogo_amd: the prediction sink lives on an MI355X device (got {device}); there is no CPU fallback")
        if mode not in _MODES:
            raise ValueError(f"invalid sink mode {mode!r}; valid modes are 'npy' and 'rows'")
        self.device, self.C, self.mode = device, int(num_classes), _MODES[mode]
        if self.mode == MODE_NPY:
            if img_hw is None:
                raise ValueError("a sink of npy records needs img_hw: the boxes are scaled to pixels")
            if self.C > 255:
                raise ValueError(f"{self.C} classes: npy records hold the class in a uint8 (at most 255)")
        self.img_h, self.img_w = (int(v) for v in img_hw) if img_hw is not None else (0, 0)
        self.reclen = (8 if self.mode == MODE_NPY else 5) + self.C
        self.flush_rows = int(flush_rows)
        self.off_rows, self.off_images, self.off_dropped, self.off_dropped_images, self.off_counts, words = state_layout(self.C)
        self.state = torch.zeros(words, dtype=torch.int64, device=device)
        self.arena: Optional[torch.Tensor] = None        # [arena_cap, reclen] fp32
        self.img_counts: Optional[torch.Tensor] = None   # [img_cap] int32
        self._images = 0          # image entries appended since the last drain (exact: one per image)
        self._rows_bound = 0      # upper bound of the records appended since the last drain
        self._rows_known = 0      # the exact total after the latest append known to have finished
        self._pending: List[Tuple[torch.cuda.Event, torch.Tensor, int]] = []   # per append: (event after it, total after it, its bound)

    # -- capacity ----------------------------------------------------------------------------------------------------------------
    def _refresh(self) -> None:
        done = None
        while self._pending and self._pending[0][0].query():
            done = self._pending.pop(0)
        if done is not None:          # its count is the total after that append; the later ones are still bounds
            self._rows_known = int(done[1])
            self._rows_bound = self._rows_known + sum(bound for _, _, bound in self._pending)

    def _reserve(self, need: int, images: int) -> None:
        """room for `need` more records and `images` more image entries.  The host knows only a bound per append (B * cap: the counts
        live on the device), so the exact total of the latest FINISHED append, copied asynchronously after each one, replaces the
        bounds up to it.  Only when the bound still does not fit is the counter itself read -- the one place where ``append`` may wait,
        and only for launches already queued; the buffer then grows if the exact count needs it.  The first buffer holds two appends'
        bounds: a caller whose batches take longer than a sink launch never waits here.  The image entries are counted exactly on
        the host; their buffer grows by a stream-ordered copy."""
        self._refresh()
        if self.arena is None:
            self.arena = torch.empty(max(2 * need, 1), self.reclen, dtype=torch.float32, device=self.device)
        if self._rows_bound + need > self.arena.shape[0]:
            exact = int(self.state[self.off_rows])
            self._pending.clear()
            self._rows_bound = self._rows_known = exact
            if exact + need > self.arena.shape[0]:
                grown = torch.empty(max(2 * self.arena.shape[0], exact + 2 * need), self.reclen, dtype=torch.float32, device=self.device)
                grown[:exact] = self.arena[:exact]
                self.arena = grown
        self._rows_bound += need
        if self.img_counts is None:
            self.img_counts = torch.empty(max(4 * images, 1024), dtype=torch.int32, device=self.device)
        if self._images + images > self.img_counts.shape[0]:
            grown = torch.empty(max(2 * self.img_counts.shape[0], self._images + 2 * images), dtype=torch.int32, device=self.device)
            grown[: self._images] = self.img_counts[: self._images]
            self.img_counts = grown
        self._images += images

    # -- per batch ---------------------------------------------------------------------------------------------------------------
    def _check(self, rows: torch.Tensor, counts: torch.Tensor) -> Tuple[int, int, int]:
        _hip.require_cuda(rows, "the kept rows")
        _hip.require_cuda(counts, "the kept-row counts")
        if rows.ndim != 3 or rows.dtype != torch.float32 or not rows.is_contiguous():
            raise ValueError(f"rows must be contiguous float32 [B, cap, 5+C], got {rows.dtype} {tuple(rows.shape)}")
        B, cap, P = rows.shape
        if P - 5 != self.C:
            raise ValueError(f"rows carry {P - 5} class scores, the sink was built for {self.C} classes")
        if counts.dtype != torch.int32 or tuple(counts.shape) != (B,) or not counts.is_contiguous():
            raise ValueError(f"counts must be int32 [{B}], got {counts.dtype} {tuple(counts.shape)}")
        return int(B), int(cap), int(P)

    def append(self, rows: torch.Tensor, counts: torch.Tensor, first_img_id: int, count_classes: bool = False) -> None:
        """compact ``rows[b, :counts[b]]`` of every image behind what the sink holds; image b gets the id ``first_img_id + b``.
        No host read (but see ``_reserve``)."""
        B, cap, P = self._check(rows, counts)
        if B == 0:
            return
        with torch.cuda.device(self.device):
            self._reserve(B * cap, B)
            ws = torch.empty(_hip.query_size("yogo_pred_sink_workspace_bytes", B), dtype=torch.uint8, device=self.device)
            _hip.call("yogo_pred_sink_append", rows, counts, B, cap, P, self.mode, int(bool(count_classes)), int(first_img_id), self.img_h,
                      self.img_w, self.state, self.arena, self.arena.shape[0], self.img_counts, self.img_counts.shape[0], ws,
                      _hip.stream_ptr())
            total = torch.empty(1, dtype=torch.int64).pin_memory()
            total.copy_(self.state[self.off_rows: self.off_rows + 1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending.append((ev, total, B * cap))

    def add_counts(self, rows: torch.Tensor, counts: torch.Tensor) -> None:
        """the counts-only call: class_counts[first argmax] += 1 per kept row whose best class score is > 0; nothing is compacted"""
        B, cap, P = self._check(rows, counts)
        if B == 0:
            return
        with torch.cuda.device(self.device):
            _hip.call("yogo_pred_sink_append", rows, counts, B, cap, P, self.mode, 1, 0, self.img_h, self.img_w, self.state, None, 0, None, 0,
                      None, _hip.stream_ptr())

    def should_flush(self) -> bool:
        """more than ``flush_rows`` records are known to be in the arena (no wait: the totals of finished appends only)"""
        self._refresh()
        return self._rows_known > self.flush_rows

    # -- read-out ----------------------------------------------------------------------------------------------------------------
    def _take(self) -> Tuple[int, int]:
        """(records, images) appended since the last drain; the totals start again at zero.  Raises if anything was dropped."""
        head = self.state[: self.off_counts].cpu()
        n, images = int(head[self.off_rows]), int(head[self.off_images])
        dropped, dropped_images = int(head[self.off_dropped]), int(head[self.off_dropped_images])
        self.state[: self.off_counts].zero_()
        self._pending.clear()
        self._rows_bound = self._rows_known = self._images = 0
        if dropped or dropped_images:
            raise RuntimeError(f"yogo_amd: the prediction sink dropped {dropped} records and {dropped_images} image entries for lack of "
                               f"room (kept {n} records of {images} images)")
        return n, images

    def drain(self) -> Tuple[np.ndarray, np.ndarray]:
        """(records float32 [N, reclen], per_image_counts int32 [images]) of everything appended since the last drain, in order;
        the totals start again at zero, ``class_counts`` go on.  Raises if anything was dropped for lack of room."""
        n, images = self._take()
        if self.arena is None or n == 0:
            records = np.zeros((0, self.reclen), dtype=np.float32)
        else:
            records = self.arena[:n].cpu().numpy()
        if self.img_counts is None or images == 0:
            per_image = np.zeros((0,), dtype=np.int32)
        else:
            per_image = self.img_counts[:images].cpu().numpy()
        return records, per_image

    def drain_text(self) -> Tuple[np.ndarray, np.ndarray]:
        """``drain()`` of a "rows" sink as text: (text uint8 [total], offsets int64 [images + 1]); ``text[offsets[k]: offsets[k + 1]]``
        are the bytes of ``prediction_rows_to_text`` of image k's rows.  The rows are formatted on the device
        (``yogo_pred_text_format``); the host reads ``total`` bytes and the offsets, not the records."""
        if self.mode != MODE_ROWS:
            raise ValueError("drain_text: prediction text is made of the kept rows; this sink holds npy records")
        n, images = self._take()
        if images == 0:
            return np.zeros((0,), dtype=np.uint8), np.zeros((1,), dtype=np.int64)
        with torch.cuda.device(self.device):
            text_bytes, ws_bytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
            _hip.call("yogo_pred_text_bound", n, images, self.reclen, ctypes.addressof(text_bytes), ctypes.addressof(ws_bytes))
            text = torch.empty(max(int(text_bytes.value), 1), dtype=torch.uint8, device=self.device)
            ws = torch.empty(max(int(ws_bytes.value), 8), dtype=torch.uint8, device=self.device)
            out = torch.empty(images + 2, dtype=torch.int64, device=self.device)   # the offsets, then the total: one copy
            _hip.call("yogo_pred_text_format", self.arena if n else None, n, self.reclen, self.img_counts, images, text, text.shape[0],
                      out, out[images + 1:], ws, _hip.stream_ptr())
            out_h = out.cpu().numpy()
            total = int(out_h[images + 1])
            if total < 0:
                raise RuntimeError(f"yogo_amd: the sink's per-image counts do not add up to its {n} records")
            if total > text.shape[0]:
                raise RuntimeError(f"yogo_amd: the prediction text needs {total} bytes, more than the bound of {text.shape[0]}")
            return text[:total].cpu().numpy(), out_h[: images + 1].copy()

    def class_counts(self) -> torch.Tensor:
        return self.state[self.off_counts: self.off_counts + self.C].cpu()
