"""Decoded training images kept resident in HBM (``yogo train --device-image-cache GIB``).

Without a cache, DataLoader workers PIL-decode every image of the split in every epoch and each stacked batch is uploaded.  With
one, each image of a split is decoded once: an ``ImageCache`` holds the uint8 pixels of split indices ``0 .. S-1`` in one
``[S, C, H, W]`` tensor on the loader's device (slot = split index, no eviction: the resident set is fixed and deterministic),
and every later batch is built there by one gather launch (yogo_amd/csrc/image_cache.hip), as uint8 or as fp32 ``/ 255`` under
``normalize_images``.  The label rows of the resident samples stay on the host, parsed once, as one flat fp32 ``[N, 5]``
tensor with int64 offsets; each batch hands them to ``format_labels_batch`` exactly as the uncached path does.

``S = min(len(real part of the split), floor(budget / (C * H * W)))``.  ``get_dataloader`` gives the budget to the train
split first and what is left to the val split; the test split is never cached.  The prefill runs before the first batch of
the split is yielded: a one-off DataLoader (``SequentialSampler`` over ``0 .. S-1``, the split's worker count, spawn, not
persistent, its own generator so that torch's global RNG -- and with it every later flip draw -- is not touched) returns
``(index, uint8 image after resize_image, label rows)`` per sample.  A sample unreadable at prefill is not made resident and
stays with the workers, which retry it every epoch as before.

``device_decode=True`` (``yogo train --device-image-decode``) fills the cache without that pool: threads read the PNG files, the
device inflates and unfilters them in chunks of ``decode_batch`` images straight into their slots (yogo_amd/png_prefill.py), and
whatever the device does not take goes through ``image_uint8`` as above.  Its scratch (pinned slots, stored streams, scanlines) is
dropped when the prefill returns and is not part of the budget.  Everything after the fill is the same code on both routes.
``device_decode_all=True`` (``--device-image-decode-all``) has that route take every PNG colour type, bit depth and Adam7 instead of
8-bit greyscale and RGB alone (yogo_amd/png_prefill.py: decode_all).  ``device_resize=True`` (``--device-image-resize``) lets that route also resize, on the device, the files whose size is not the
cache's (csrc/resize_aa.hip); a few of their pixels may then differ by one grey level from ``resize_image``'s (png_prefill.py).

The one deliberate difference to the uncached path: a resident image is a snapshot taken at prefill, so a file changed or
removed later is still served.  Otherwise pixels and labels are bit-identical.
"""
from __future__ import annotations

import bisect
import math
import time
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch.utils.data import ConcatDataset, DataLoader, Dataset, SequentialSampler, Subset

from yogo_amd import _hip, png_prefill
from yogo_amd.png_prefill import DEFAULT_DECODE_BATCH
from yogo_amd.yogo_dataset import ObjectDetectionDataset

GIB = 2 ** 30
FLAG = "--device-image-cache"
DECODE_FLAG = "--device-image-decode"
RESIZE_FLAG = "--device-image-resize"
DECODE_ALL_FLAG = "--device-image-decode-all"
DECODE_JPEG_FLAG = "--device-image-decode-jpeg"


def check_budget_gib(gib: float) -> float:
    """the budget in GiB as a float; ValueError unless it is a finite number > 0"""
    try:
        x = float(gib)
    except (TypeError, ValueError):
        raise ValueError(f"{FLAG}: {gib!r} is not a number of GiB") from None
    if not (math.isfinite(x) and x > 0):
        raise ValueError(f"{FLAG}: the budget must be a finite number of GiB > 0, got {gib!r}")
    return x


def budget_bytes(gib: float) -> int:
    """GiB (2^30 bytes) -> whole bytes, rounded down"""
    return int(math.floor(check_budget_gib(gib) * GIB))


def resident_count(budget: int, split_len: int, C: int, H: int, W: int) -> int:
    """S = min(split size, floor(budget bytes / (C * H * W)))"""
    return max(0, min(int(split_len), int(budget) // (C * H * W)))


def resolve_sample(dataset: Dataset, index: int) -> Tuple[ObjectDetectionDataset, int]:
    """split index -> (the ObjectDetectionDataset that holds it, its index there), through Subset / ConcatDataset"""
    index = int(index)
    while True:
        if isinstance(dataset, ObjectDetectionDataset):
            return dataset, index
        if isinstance(dataset, Subset):
            index = int(dataset.indices[index])
            dataset = dataset.dataset
        elif isinstance(dataset, ConcatDataset):
            k = bisect.bisect_right(dataset.cumulative_sizes, index)
            if k:
                index -= dataset.cumulative_sizes[k - 1]
            dataset = dataset.datasets[k]
        else:
            raise TypeError(f"{FLAG}: cannot resolve a sample of {type(dataset).__name__} (only ObjectDetectionDataset behind "
                            "Subset / ConcatDataset is cached)")


class ResidentIndex(int):
    """What a worker hands over for a resident sample: its split index (the image is gathered on the device)."""

    def __repr__(self) -> str:
        return f"ResidentIndex({int(self)})"


class ResidentMarkers(Dataset):
    """What the workers see of a partially resident split: a ``ResidentIndex`` for a resident index, exactly what the split
    returns today for every other one.  ``resident`` is the cache's flag array; it is final before the workers start (the
    prefill runs before the split's first iteration) and travels with the pickled wrapper."""

    def __init__(self, dataset: Dataset, resident: np.ndarray):
        self.dataset = dataset
        self.resident = resident

    def __len__(self) -> int:
        return len(self.dataset)   # type: ignore[arg-type]

    def __getitem__(self, i: int):
        if 0 <= i < len(self.resident) and self.resident[i]:
            return ResidentIndex(i)
        return self.dataset[i]


def collate_cached(batch: List) -> Optional[Tuple[Optional[torch.Tensor], List[torch.Tensor], List[int], List[int], List[int],
                                                  List[int], List[int], int]]:
    """``collate_mixed`` for batches that may also hold resident samples: unreadable samples (None) are dropped and the rest
    close up, in the sampler's order.  -> (uploaded images stacked or None, their label rows, their batch rows, resident split
    indices, their batch rows, blob indices, their batch rows, batch size); None when nothing is left."""
    imgs: List[torch.Tensor] = []
    rows: List[torch.Tensor] = []
    up_pos: List[int] = []
    res_idx: List[int] = []
    res_pos: List[int] = []
    blob_idx: List[int] = []
    blob_pos: List[int] = []
    b = 0
    for item in batch:
        if item is None:
            continue
        if isinstance(item, ResidentIndex):
            res_idx.append(int(item))
            res_pos.append(b)
        elif isinstance(item, int):
            blob_idx.append(item)
            blob_pos.append(b)
        else:
            imgs.append(item[0])
            rows.append(item[1])
            up_pos.append(b)
        b += 1
    if b == 0:
        return None
    return (torch.stack(imgs) if imgs else None), rows, up_pos, res_idx, res_pos, blob_idx, blob_pos, b


class _PrefillItems(Dataset):
    """split index i -> (i, uint8 image after resize_image or None when unreadable, label rows or None)"""

    def __init__(self, split: Dataset, S: int):
        self.split, self.S = split, int(S)

    def __len__(self) -> int:
        return self.S

    def __getitem__(self, i: int):
        ds, j = resolve_sample(self.split, i)
        img = ds.image_uint8(j)
        return int(i), img, (ds.label_rows(j) if img is not None else None)


def _collate_prefill(batch):
    kept = [(i, img, rows) for i, img, rows in batch if img is not None]
    return [i for i, _, _ in kept], (torch.stack([img for _, img, _ in kept]) if kept else None), [rows for _, _, rows in kept]


def gather(cache: torch.Tensor, slots: Union[Sequence[int], torch.Tensor], out: torch.Tensor) -> torch.Tensor:
    """out[b] = cache[slots[b]] for every b with slots[b] >= 0 (uint8, or fp32 x / 255 when out is fp32), one launch; rows with
    a negative slot are left as they are.  cache: contiguous uint8 [S, C, H, W]; out: contiguous [B, C, H, W] uint8 or fp32 on
    the same device; every slot < S (checked here, before the launch)."""
    _hip.require_cuda(cache, "the image cache")
    _hip.require_cuda(out, "the gather output")
    if cache.dtype != torch.uint8 or cache.ndim != 4 or not cache.is_contiguous() or cache.shape[0] == 0:
        raise ValueError(f"gather: the cache must be a non-empty contiguous uint8 [S, C, H, W] tensor, got {tuple(cache.shape)} {cache.dtype}")
    if (out.dtype not in (torch.uint8, torch.float32) or out.ndim != 4 or tuple(out.shape[1:]) != tuple(cache.shape[1:])
            or not out.is_contiguous()):
        raise ValueError(f"gather: out must be a contiguous [B, {', '.join(map(str, cache.shape[1:]))}] uint8 or float32 tensor, "
                         f"got {tuple(out.shape)} {out.dtype}")
    if out.device != cache.device:
        raise ValueError(f"gather: the cache is on {cache.device}, out on {out.device}")
    S, (B, C, H, W) = int(cache.shape[0]), out.shape
    if S >= 2 ** 31:
        raise ValueError(f"gather: {S} cache slots, at most 2^31 - 1")
    sl = torch.as_tensor(slots, dtype=torch.int64).reshape(-1).cpu()
    if sl.numel() != B:
        raise ValueError(f"gather: {sl.numel()} slots for {B} batch rows")
    if B and int(sl.max()) >= S:
        raise IndexError(f"gather: slot {int(sl.max())} is out of range for a cache of {S} images")
    if B == 0:
        return out
    with torch.cuda.device(out.device):
        _hip.call("yogo_image_cache_gather", cache, S, sl.clamp(min=-1).to(torch.int32).to(out.device, non_blocking=True), B, C, H, W,
                  out, 1 if out.dtype == torch.float32 else 0, _hip.stream_ptr())
    return out


class ImageCache:
    """The resident images of one split: split indices 0 .. S-1 in slots 0 .. S-1 of one uint8 [S, C, H, W] device tensor,
    plus their label rows on the host.  Allocated at construction, filled by ``prefill()`` (once, before the split's first
    batch).  ``split`` is the split as get_datasets made it (a thumbnail-augmented one included: only indices < S, which lie
    in its real part, are cached)."""

    def __init__(self, split: Dataset, S: int, image_shape: Tuple[int, int, int], normalize_images: bool, device=None,
                 num_workers: int = 0, batch_size: int = 64, name: str = "train", log: bool = False, device_decode: bool = False,
                 decode_batch: int = DEFAULT_DECODE_BATCH, device_resize: bool = False, device_decode_all: bool = False,
                 device_decode_jpeg: bool = False):
        if device_resize and not device_decode:
            raise ValueError(f"{RESIZE_FLAG} resizes what the device decoded: it needs {DECODE_FLAG}")
        if device_decode_all and not device_decode:
            raise ValueError(f"{DECODE_ALL_FLAG} widens what {DECODE_FLAG} takes: it needs {DECODE_FLAG}")
        if device_decode_jpeg and not device_decode:
            raise ValueError(f"{DECODE_JPEG_FLAG} widens what {DECODE_FLAG} takes: it needs {DECODE_FLAG}")
        if not torch.cuda.is_available():
            raise RuntimeError(f"yogo_amd: {FLAG} keeps images on an MI355X device; there is no CPU fallback")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError(f"yogo_amd: {FLAG} keeps images on an MI355X device (got {dev}); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        C, H, W = (int(v) for v in image_shape)
        self.split, self.S, self.image_shape = split, int(S), (C, H, W)
        self.split_len = len(split)   # type: ignore[arg-type]
        if not 0 < self.S <= self.split_len:
            raise ValueError(f"ImageCache: S = {S} outside [1, {self.split_len}]")
        self.normalize_images, self.device = bool(normalize_images), dev
        self.num_workers, self.batch_size, self.name, self.log = int(num_workers), max(1, int(batch_size)), name, log
        self.device_decode, self.decode_batch = bool(device_decode), png_prefill.check_decode_batch(decode_batch)
        self.device_resize, self.device_decode_all = bool(device_resize), bool(device_decode_all)
        self.device_decode_jpeg = bool(device_decode_jpeg)
        self.decode_stats: dict = {}   # what png_prefill.fill reports of a device prefill (chunk times, scratch bytes); empty otherwise
        self.nbytes = self.S * C * H * W
        try:
            self.images = torch.empty((self.S, C, H, W), dtype=torch.uint8, device=dev)
        except RuntimeError as e:   # torch.OutOfMemoryError included
            raise RuntimeError(f"yogo_amd: {FLAG}: could not allocate {self.nbytes} bytes on {dev} for {self.S} images of the "
                               f"{name} split ({e})") from e
        self.resident = np.zeros(self.S, dtype=bool)
        self.rows = torch.zeros(0, 5, dtype=torch.float32)
        self.row_offsets = np.zeros(self.S + 1, dtype=np.int64)
        self.prefilled = False
        self.prefill_seconds = 0.0

    @property
    def full(self) -> bool:
        """every index of the split is resident: its batches need no worker"""
        return self.prefilled and self.S == self.split_len and bool(self.resident.all())

    def label_rows(self, index: int) -> torch.Tensor:
        """the [N, 5] label rows of resident split index `index` (a view of the host arena)"""
        return self.rows[int(self.row_offsets[index]):int(self.row_offsets[index + 1])]

    def prefill(self) -> None:
        """decode split indices 0 .. S-1 once and copy them into their slots (no-op after the first call)"""
        if self.prefilled:
            return
        t0 = time.perf_counter()
        with torch.cuda.device(self.device):
            rows = self._fill_on_device() if self.device_decode else self._fill_from_workers()
            torch.cuda.synchronize(self.device)
        for i, r in enumerate(rows):
            self.resident[i] = r is not None
        counts = np.array([0 if r is None else int(r.shape[0]) for r in rows], dtype=np.int64)
        self.row_offsets = np.zeros(self.S + 1, dtype=np.int64)
        self.row_offsets[1:] = np.cumsum(counts)
        kept = [r for r in rows if r is not None and r.shape[0]]
        self.rows = torch.cat(kept) if kept else torch.zeros(0, 5, dtype=torch.float32)
        self.prefilled = True
        self.prefill_seconds = dt = time.perf_counter() - t0
        n = int(self.resident.sum())
        if self.log:
            print(f"yogo_amd: device image cache ({self.name}): {n} of {self.split_len} images resident, {self.nbytes} bytes of HBM; "
                  f"prefill {dt:.2f} s ({n / max(dt, 1e-9):.0f} images/s)", flush=True)

    def _fill_from_workers(self) -> List[Optional[torch.Tensor]]:
        """the host route: a one-off DataLoader decodes, the pixels are copied up -> per slot its label rows, None = not resident"""
        items = _PrefillItems(self.split, self.S)
        nw = self.num_workers
        loader = DataLoader(items, batch_size=self.batch_size, sampler=SequentialSampler(items), num_workers=nw, persistent_workers=False,
                            pin_memory=True, collate_fn=_collate_prefill, generator=torch.Generator().manual_seed(0),
                            multiprocessing_context="spawn" if nw > 0 else None)
        rows: List[Optional[torch.Tensor]] = [None] * self.S
        for idx, imgs, rws in loader:
            if not idx:
                continue
            slots = torch.tensor(idx, dtype=torch.long).to(self.device, non_blocking=True)
            self.images.index_copy_(0, slots, imgs.to(self.device, non_blocking=True))
            for i, r in zip(idx, rws):
                rows[i] = r.reshape(-1, 5).to(torch.float32)
        return rows

    def _fill_on_device(self) -> List[Optional[torch.Tensor]]:
        """the device route (yogo_amd/png_prefill.py): the same result, the PNG files inflated and unfiltered on the device"""
        return png_prefill.fill(self.images, [resolve_sample(self.split, i) for i in range(self.S)], self.decode_batch, self.decode_stats,
                                device_resize=self.device_resize, **({"decode_all": True} if self.device_decode_all else {}),
                                **({"decode_jpeg": True} if self.device_decode_jpeg else {}))
