"""``BlobDataset`` -- synthetic training images made of cell thumbnails (yogo/data/blobgen.py), composed on the MI355X.

A blob image is a background of flat shade with up to ``n`` randomly drawn thumbnails pasted at non-overlapping positions,
and its label tensor.  The reference builds one per ``__getitem__`` inside DataLoader workers; here construction is the only
host work (list and decode the thumbnails once, compute their shades) and a whole batch of blob images is three HIP launches
(yogo_amd/csrc/blobgen.hip) plus the label rasteriser, written straight into the rows of the caller's batch tensor.

Kept from the reference: the constructor's arguments; class keys given as names or indices; ``FileNotFoundError`` for a
missing directory; ``*.png`` files of each directory (not recursive, names starting with ``.`` skipped) read as grayscale;
the strict ``h * w > 500`` filter; the shade of a thumbnail (``get_background_shade``); ``n`` draws with replacement over all
thumbnails; the background = the truncated mean shade of all ``n`` draws; per thumbnail a horizontal and a vertical flip with
p = 0.5 each and up to 100 tries for a position whose box intersects no box accepted so far (touching edges allowed), else
the thumbnail is skipped; label rows ``(class, x/W, y/H, (x+w)/W, (y+h)/H)`` in placement order, rasterised as xyxy;
``normalize_images`` -> ``img / 255`` in fp32.

Deliberate differences:

* **Randomness.**  The reference draws from numpy's global state inside workers, which no run can reproduce.  Here every
  draw is a pure function of ``(seed, epoch, dataset index, thumbnail slot, draw kind, try)`` through a counter-based hash
  (splitmix64's output function; the exact rule is at the top of blobgen.hip).  A blob image therefore does not depend on
  the worker count, the rank or the other images of its batch, and tests/_blobgen_ref.py restates the generator exactly.
  The thumbnails of a directory are taken in sorted file-name order (the reference's glob order is the file system's).
* **Thumbnails that cannot fit.**  A thumbnail with ``h >= H`` or ``w >= W`` makes the reference crash in
  ``np.random.randint``; here it is refused at construction with a ``ValueError`` naming the file.
* **No thumbnails.**  If no thumbnail survives the filter, a ``FileNotFoundError`` says so (the reference's intent).
* **n is capped** at ``BLOB_MAX_N`` = 256: the placement kernel holds the accepted boxes of an image in LDS.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import torch
from torch.utils.data import Dataset

from yogo_amd import _hip
from yogo_amd.data import LABEL_TENSOR_PRED_DIM_SIZE

PathLike = Union[str, Path]

BLOB_MAX_N = 256        # blobgen.hip: BLOB_MAX_N
AREA_THRESHOLD = 500    # blobgen.py:66 (strict: h * w > 500)
BRIGHTNESS_THRESHOLD = 210


def background_shade(thumbnail: torch.Tensor, brightness_threshold: int = BRIGHTNESS_THRESHOLD) -> int:
    """blobgen.py:168-179 (get_background_shade): the mean of the pixels brighter than 210, 210 if there are none, truncated."""
    return int(thumbnail[thumbnail > brightness_threshold].float().mean().nan_to_num(brightness_threshold).item())


class BlobDataset(Dataset):
    """Synthetic images from thumbnails, blobgen.py:23-263.  Construction is host-only (no HIP call: CPU code and spawn
    workers can build and pickle it); the thumbnails move to a device on first use there."""

    def __init__(self, thumbnail_dir_paths: Mapping[Union[str, int], Union[PathLike, List[PathLike]]], Sx: int, Sy: int,
                 classes: List[str], n: int = 50, length: int = 1000, background_img_shape: Tuple[int, int] = (772, 1032),
                 normalize_images: bool = False, seed: int = 0):
        super().__init__()
        if not 1 <= int(n) <= BLOB_MAX_N:
            raise ValueError(f"BlobDataset: n = {n} thumbnails per image is outside [1, {BLOB_MAX_N}] (the placement kernel keeps "
                             f"the accepted boxes of an image in LDS)")
        self.thumbnail_dir_paths: Dict[int, List[Path]] = {
            self._convert_label(k, classes): [Path(vv) for vv in (v if isinstance(v, (list, tuple)) else [v])]
            for k, v in thumbnail_dir_paths.items()}
        for dirs in self.thumbnail_dir_paths.values():
            for d in dirs:
                if not d.exists():
                    raise FileNotFoundError(f"{d} does not exist")
        self.Sx, self.Sy, self.n, self.length = Sx, Sy, int(n), int(length)
        self.background_img_shape = (int(background_img_shape[0]), int(background_img_shape[1]))
        self.normalize_images = normalize_images
        self.seed = int(seed)
        self.area_threshold = AREA_THRESHOLD
        self._load(self.thumbnail_dir_paths)
        self._device_tables: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}

    @staticmethod
    def _convert_label(label: Union[str, int], classes: List[str]) -> int:
        """blobgen.py:114-123"""
        if isinstance(label, int):
            if not 0 <= label < len(classes):
                raise ValueError(f"label {label} is out of range [0, {len(classes)})")
            return label
        if label not in classes:
            raise ValueError(f"label {label} is not a valid YOGO class")
        return classes.index(label)

    def _load(self, dir_paths: Dict[int, List[Path]]) -> None:
        """blobgen.py:82-112, :128-149: every thumbnail of every class, decoded once; the strict area filter; the shades"""
        from yogo_amd.yogo_dataset import read_image_robust

        pairs: List[Tuple[int, Path]] = []
        for cls, dirs in dir_paths.items():
            for d in dirs:
                pairs.extend((cls, p) for p in sorted(d.glob("*.png")) if not p.name.startswith("."))
        with ThreadPoolExecutor(max_workers=8) as ex:
            images = list(ex.map(read_image_robust, [p for _, p in pairs]))
        H, W = self.background_img_shape
        kept = [(cls, p, t) for (cls, p), t in zip(pairs, images) if t is not None and t.shape[1] * t.shape[2] > self.area_threshold]
        if not kept:
            raise FileNotFoundError(f"no thumbnails (*.png with more than {self.area_threshold} pixels) found in any of "
                                    f"{[str(d) for dirs in dir_paths.values() for d in dirs]}")
        for _, p, t in kept:
            if t.shape[1] >= H or t.shape[2] >= W:
                raise ValueError(f"thumbnail {p} is {t.shape[1]} x {t.shape[2]}: it cannot be placed in a {H} x {W} image")
        self.thumbnail_paths = [p for _, p, _ in kept]
        self.classes = torch.tensor([cls for cls, _, _ in kept], dtype=torch.int32)
        self.thumbnail_dims = torch.tensor([[t.shape[1], t.shape[2]] for _, _, t in kept], dtype=torch.int32)
        self.shades = torch.tensor([background_shade(t) for _, _, t in kept], dtype=torch.int32)
        sizes = self.thumbnail_dims[:, 0].long() * self.thumbnail_dims[:, 1].long()
        offsets = torch.zeros(len(kept), dtype=torch.long)
        offsets[1:] = sizes.cumsum(0)[:-1]
        if int(sizes.sum()) >= 2 ** 31:
            raise ValueError("BlobDataset: the thumbnails hold more than 2^31 pixels")
        self.atlas = torch.cat([t.reshape(-1) for _, _, t in kept]).contiguous()
        # [T][5] int32: atlas offset, h, w, class, shade (include/yogo_hip.h, yogo_blobgen_place)
        self.table = torch.stack([offsets.int(), self.thumbnail_dims[:, 0], self.thumbnail_dims[:, 1], self.classes, self.shades], 1).contiguous()
        self.num_thumbnails = len(kept)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_device_tables"] = {}
        return state

    def __len__(self) -> int:
        return self.length

    def _tables(self, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        """the atlas and the table on `dev`, uploaded once"""
        if dev not in self._device_tables:
            self._device_tables[dev] = (self.atlas.to(dev), self.table.to(dev))
        return self._device_tables[dev]

    @staticmethod
    def _device(out_imgs: Optional[torch.Tensor]) -> torch.device:
        if out_imgs is not None:
            _hip.require_cuda(out_imgs, "the output image batch")
            return out_imgs.device
        if not torch.cuda.is_available():
            raise RuntimeError("yogo_amd: blob images are composed on an MI355X device; there is no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())

    def _indices(self, indices: Union[Sequence[int], torch.Tensor]) -> torch.Tensor:
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).cpu()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.length):
            raise IndexError(f"blob indices must lie in [0, {self.length})")
        return idx.int()

    def place(self, indices: Union[Sequence[int], torch.Tensor], epoch: int = 0, device=None
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The draws and the placement of images `indices` in `epoch`: device (boxes [S, n, 4] int32 = (thumbnail, x, y,
        flips: bit 0 horizontal, bit 1 vertical), rows [S, n, 5] fp32, counts [S] int32, background [S] int32)."""
        dev = torch.device(device) if device is not None else self._device(None)
        idx = self._indices(indices)
        S, n = int(idx.numel()), self.n
        H, W = self.background_img_shape
        _, table = self._tables(dev)
        with torch.cuda.device(dev):
            boxes = torch.empty(S, n, 4, dtype=torch.int32, device=dev)
            rows = torch.empty(S, n, 5, dtype=torch.float32, device=dev)
            counts = torch.empty(S, dtype=torch.int32, device=dev)
            background = torch.empty(S, dtype=torch.int32, device=dev)
            if S:
                _hip.call("yogo_blobgen_place", table, self.num_thumbnails, idx.to(dev), S, n, H, W, self.seed & 0xFFFFFFFF,
                          int(epoch) & 0xFFFFFFFF, boxes, rows, counts, background, _hip.stream_ptr())
        return boxes, rows, counts, background

    def generate(self, indices: Union[Sequence[int], torch.Tensor], epoch: int = 0, out_imgs: Optional[torch.Tensor] = None,
                 positions: Optional[Union[Sequence[int], torch.Tensor]] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Blob images `indices` of `epoch` on the device: (imgs [S, 1, H, W] uint8, or fp32 with normalize_images; labels
        [S, 6, Sy, Sx]; rows [S, n, 5]; counts [S]).  With `out_imgs` ([B, 1, H, W], contiguous) image s is written into
        out_imgs[positions[s]] and `imgs` is `out_imgs`; no host synchronisation."""
        dev = self._device(out_imgs)
        H, W = self.background_img_shape
        dtype = torch.float32 if self.normalize_images else torch.uint8
        S = len(indices)
        if out_imgs is None:
            if positions is not None:
                raise ValueError("generate: positions without out_imgs")
            out_imgs = torch.empty(S, 1, H, W, dtype=dtype, device=dev)
            pos = torch.arange(S, dtype=torch.int32)
        else:
            if out_imgs.ndim != 4 or tuple(out_imgs.shape[1:]) != (1, H, W) or out_imgs.dtype != dtype or not out_imgs.is_contiguous():
                raise ValueError(f"generate: out_imgs must be a contiguous [B, 1, {H}, {W}] {dtype} tensor, got "
                                 f"{tuple(out_imgs.shape)} {out_imgs.dtype}")
            pos = torch.as_tensor(positions if positions is not None else list(range(S)), dtype=torch.int64).reshape(-1).cpu()
            if pos.numel() != S or (S and (int(pos.min()) < 0 or int(pos.max()) >= out_imgs.shape[0])):
                raise ValueError(f"generate: need {S} positions in [0, {out_imgs.shape[0]})")
            pos = pos.int()
        boxes, rows, counts, background = self.place(indices, epoch, dev)
        atlas, table = self._tables(dev)
        with torch.cuda.device(dev):
            labels = torch.empty(S, LABEL_TENSOR_PRED_DIM_SIZE, self.Sy, self.Sx, dtype=torch.float32, device=dev)
            if S:
                stream = _hip.stream_ptr()
                _hip.call("yogo_blobgen_compose", atlas, atlas.numel(), table, boxes, counts, background, pos.to(dev), S, self.n, H, W,
                          out_imgs, out_imgs.element_size(), stream)
                flat = torch.empty(S * self.n, 5, dtype=torch.float32, device=dev)
                offsets = torch.empty(S + 1, dtype=torch.int32, device=dev)
                _hip.call("yogo_blobgen_label_rows", rows, counts, S, self.n, flat, offsets, stream)
                # (every placed box lies inside the image, so its cell lies inside the grid: the status stays 0 and is not read)
                status = torch.zeros(1, dtype=torch.int32, device=dev)
                _hip.call("yogo_labels_rasterize", flat, offsets, labels, status, S, self.Sx, self.Sy, 0, stream)
        return out_imgs, labels, rows, counts

    def __getitem__(self, idx: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """blobgen.py:208-263: (img [1, H, W], labels [6, Sy, Sx]) on the current device, epoch 0"""
        if idx >= self.length:
            raise IndexError(f"index {idx} is out of bounds for length {self.length}")
        imgs, labels, _, _ = self.generate([idx], 0)
        return imgs[0], labels[0]
