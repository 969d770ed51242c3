"""Datasets -> batches on the device (yogo/data/yogo_dataloader.py:69-324).

``get_datasets`` / ``split_dataset`` / ``get_dataloader`` keep the reference's names, arguments and split behaviour
(``random_split`` under ``manual_seed(7271978)``, ``DistributedSampler`` per rank with torch's defaults, batch-level flip
augmentations on the training split only).  What differs is WHERE the work happens: workers decode images and parse label
files, the loader then moves the stacked uint8 images to the MI355X, rasterises all label tensors of the batch with one HIP
launch and applies both flips in one fused pass (yogo_amd/data.py) -- a ``DeviceLoader`` yields ``(imgs [B,C,H,W] uint8,
labels [B,6,Sy,Sx] fp32)`` already resident in HBM, which is what ``HipTrainer.step`` consumes.

Thumbnail augmentation (``thumbnail_augmentation:`` in the definition, yogo_dataloader.py:137-152): the train split gets a
``BlobDataset`` of ``len(train) // 2`` synthetic images appended, shuffled with the real ones by the sampler.  Workers never
make a synthetic image: for its indices they hand over the index alone (``BlobIndices``), and ``DeviceLoader`` composes those
images on the device straight into their rows of the batch (yogo_amd/blobgen.py), with ``epoch = sampler.epoch``.  A
definition without the key takes exactly the path above.

Device image cache (``device_image_cache_gib``, ``yogo train --device-image-cache GIB``; yogo_amd/image_cache.py): the train
split, then the val split with what is left of the budget, keeps split indices ``0 .. S-1`` decoded in HBM.  A fully
resident split starts no worker at all: ``DeviceLoader`` walks the sampler's indices in batches and gathers them on the
device.  A partially resident one hands the workers a ``ResidentMarkers`` wrapper, and each batch is assembled from uploaded,
resident and blob rows.  ``device_image_decode`` (``--device-image-decode``) fills the cache from PNG files decoded on the device
(yogo_amd/png_prefill.py); the batches are the same.  ``device_image_resize`` (``--device-image-resize``) has that route resize
files of another size than ``image_hw`` on the device too (a few pixels of those may differ by one grey level);
``device_image_decode_all`` (``--device-image-decode-all``) has it take every PNG colour type, bit depth and Adam7.  Without a budget nothing of this exists: the same ``DeviceLoader`` path, no allocation, no prefill.

Device image stream (``device_image_stream``, ``yogo train | test --device-image-stream``; yogo_amd/image_stream.py): what is
file-backed and not resident -- every split without a cache, the test split always -- is decoded on the device as well, every epoch,
in groups of ``stream_decode_batch`` images that land in a staging tensor; ``DeviceLoader`` takes its items from the stream instead
of the host DataLoader (which is never iterated: no workers) and gathers the streamed rows from the staging next to the cache's
resident rows and the blob rows.  The two widening switches then widen the stream as they widen the prefill.  Off (the default),
nothing of it exists.
"""
from __future__ import annotations

import contextlib
import os
import warnings
from typing import Any, Dict, Iterable, List, MutableMapping, Optional, Tuple

import torch
from torch.utils.data import ConcatDataset, DataLoader, Dataset, Subset, random_split
from torch.utils.data.distributed import DistributedSampler

from yogo_amd.blobgen import BlobDataset
from yogo_amd.data import MultiArgSequential, RandomHorizontalFlipWithBBs, RandomVerticalFlipWithBBs, format_labels_batch
from yogo_amd.dataset_definition_file import DatasetDefinition, SplitFractions
from yogo_amd.image_stream import ImageStream, Scratch, Staged
from yogo_amd.image_cache import DECODE_ALL_FLAG, DECODE_FLAG, DECODE_JPEG_FLAG, FLAG, RESIZE_FLAG, ImageCache, ResidentMarkers, budget_bytes, collate_cached, gather, resident_count
from yogo_amd.png_prefill import DEFAULT_DECODE_BATCH
from yogo_amd.yogo_dataset import ObjectDetectionDataset

SPLIT_SEED = 7271978   # yogo/data/yogo_dataloader.py:176

_stream_scope = (False, False, False)   # device_image_stream, device_image_decode_all, device_image_resize
_stream_jpeg = False                    # device_image_decode_jpeg, inside a stream scope


@contextlib.contextmanager
def device_image_stream_scope(enabled: bool, decode_all: bool = False, resize: bool = False):
    """every ``get_dataloader`` call inside runs with ``device_image_stream=True`` when `enabled` (and then with the two widening
    switches as given): how ``yogo test --device-image-stream`` reaches the call that ``yogo_amd.utils.test_model`` makes with the
    reference's arguments, as ``trainer.device_metrics_scope`` does for ``--device-metrics``"""
    global _stream_scope
    prev = _stream_scope
    if enabled:
        _stream_scope = (True, bool(decode_all) or prev[1], bool(resize) or prev[2])
    try:
        yield
    finally:
        _stream_scope = prev


@contextlib.contextmanager
def device_image_jpeg_scope(enabled: bool):
    """inside a ``device_image_stream_scope``: the stream decodes baseline JPEG files on the device as well (``yogo test
    --device-image-stream --device-image-decode-jpeg``)"""
    global _stream_jpeg
    prev = _stream_jpeg
    _stream_jpeg = bool(enabled) or prev
    try:
        yield
    finally:
        _stream_jpeg = prev


def guess_suggested_num_workers() -> Optional[int]:
    if hasattr(os, "sched_getaffinity"):
        try:
            return len(os.sched_getaffinity(0))
        except Exception:
            pass
    n = os.cpu_count()
    if n is None:
        warnings.warn("could not figure out the number of cpus on this machine")
    return n


def choose_dataloader_num_workers(dataset_size: int, requested_num_workers: Optional[int] = None) -> int:
    if dataset_size < 1000:
        return 0
    if requested_num_workers is not None:
        return requested_num_workers
    return min(guess_suggested_num_workers() or 32, 64)


def _concat(dataset_paths, Sx, Sy, classes, image_hw, rgb, normalize_images) -> ConcatDataset:
    return ConcatDataset([ObjectDetectionDataset(dsp.image_path, dsp.label_path, Sx, Sy, image_hw=image_hw, rgb=rgb, classes=classes,
                                                 normalize_images=normalize_images) for dsp in dataset_paths])


def get_datasets(dataset_definition: DatasetDefinition, Sx: int, Sy: int, rgb: bool = False, image_hw: Tuple[int, int] = (772, 1032),
                 normalize_images: bool = False, split_fraction_override: Optional[SplitFractions] = None) -> MutableMapping[str, Dataset]:
    """dataset definition -> {"train": ..., "val": ..., "test": ...} (yogo_dataloader.py:69-152).  With thumbnail augmentation
    the train split is ``ConcatDataset([train, BlobDataset(n=100, length=len(train) // 2)])``, as in the reference; it is
    refused together with ``rgb`` (the reference then fails at collate: 1-channel blob images beside 3-channel ones)."""
    thumbnails = getattr(dataset_definition, "thumbnail_augmentation", None)
    if thumbnails and rgb:
        raise ValueError("thumbnail_augmentation makes grayscale images; it cannot be combined with rgb")
    classes = dataset_definition.classes
    full = _concat(dataset_definition.dataset_paths, Sx, Sy, classes, image_hw, rgb, normalize_images)
    test_paths = dataset_definition.test_dataset_paths
    if test_paths is not None and len(test_paths) > 0:
        test = _concat(test_paths, Sx, Sy, classes, image_hw, rgb, normalize_images)
        if split_fraction_override is not None:
            split = split_dataset(ConcatDataset([full, test]), split_fraction_override)
        else:
            assert "test" not in dataset_definition.split_fractions
            split = {**split_dataset(full, dataset_definition.split_fractions), "test": test}
    else:
        split = split_dataset(full, split_fraction_override if split_fraction_override is not None else dataset_definition.split_fractions)
    if thumbnails:
        bd = BlobDataset(thumbnails, Sx=Sx, Sy=Sy, classes=classes, n=100, length=len(split["train"]) // 2,   # type: ignore[arg-type]
                         background_img_shape=tuple(image_hw), normalize_images=normalize_images)
        split["train"] = ConcatDataset([split["train"], bd])
    return split


def split_dataset(dataset: Dataset, split_fractions: SplitFractions) -> MutableMapping[str, Dataset]:
    if not hasattr(dataset, "__len__"):
        raise ValueError(f"dataset {dataset} must have a length (specifically, `__len__` must be defined)")
    keys = split_fractions.keys()
    sizes = split_fractions.partition_sizes(len(dataset))   # type: ignore[arg-type]
    return dict(zip(keys, random_split(dataset, [sizes[k] for k in keys], generator=torch.Generator().manual_seed(SPLIT_SEED))))


def collate_rows(batch: List[Optional[Tuple[torch.Tensor, torch.Tensor]]]) -> Optional[Tuple[torch.Tensor, List[torch.Tensor]]]:
    """host side of yogo/data/utils.py:49-63 (collate_batch_robust): drop unreadable samples, stack the images; the label rows stay
    a list (ragged) until the device rasterises them"""
    pairs = [pair for pair in batch if pair is not None]
    if not pairs:
        return None
    imgs, rows = zip(*pairs)
    return torch.stack(imgs), list(rows)


class BlobIndices(Dataset):
    """What the workers see of a ``BlobDataset``: item i is the index i itself (the image is made on the device)."""

    def __init__(self, length: int):
        self.length = length

    def __len__(self) -> int:
        return self.length

    def __getitem__(self, i: int) -> int:
        if not 0 <= i < self.length:
            raise IndexError(f"index {i} is out of bounds for length {self.length}")
        return int(i)


def collate_mixed(batch: List[Any]) -> Optional[Tuple[Optional[torch.Tensor], List[torch.Tensor], List[int], List[int], List[int], int]]:
    """``collate_rows`` for batches of real samples and blob indices (ints), in the sampler's order: unreadable real samples
    are dropped and the rest close up.  -> (real images stacked or None, their label rows, their batch rows, blob indices,
    their batch rows, batch size); None when nothing is left."""
    imgs: List[torch.Tensor] = []
    rows: List[torch.Tensor] = []
    real_pos: List[int] = []
    blob_idx: List[int] = []
    blob_pos: List[int] = []
    b = 0
    for item in batch:
        if item is None:
            continue
        if isinstance(item, int):
            blob_idx.append(item)
            blob_pos.append(b)
        else:
            imgs.append(item[0])
            rows.append(item[1])
            real_pos.append(b)
        b += 1
    if b == 0:
        return None
    return (torch.stack(imgs) if imgs else None), rows, real_pos, blob_idx, blob_pos, b


class DeviceLoader:
    """wraps the host DataLoader: batch -> device, label rows -> [B, 6, Sy, Sx] with one launch, flips fused.  Keeps the
    attributes the training loop touches (``dataset``, ``sampler``, ``batch_size``, ``__len__``)."""

    def __init__(self, loader: DataLoader, Sx: int, Sy: int, transforms: MultiArgSequential, device=None, strict_steps: bool = False,
                 blob: Optional[BlobDataset] = None, dataset: Optional[Dataset] = None, cache: Optional[ImageCache] = None,
                 stream: Optional[ImageStream] = None, normalize_images: bool = False):
        self.loader, self.Sx, self.Sy, self.transforms, self.device = loader, Sx, Sy, transforms, device
        # strict_steps (the TRAINING split only): every batch is one gradient all-reduce, so a skipped batch must fail loudly
        # under data parallelism; validation / test loaders issue no per-step collective and may skip, as the reference does
        self.strict_steps = strict_steps
        # blob: the BlobDataset behind the BlobIndices of a thumbnail-augmented train split (loader.collate_fn = collate_mixed);
        # dataset: the split as get_datasets made it (the loader iterates its worker-side form)
        self.blob = blob
        # cache: the resident images of the split (loader.dataset = ResidentMarkers, loader.collate_fn = collate_cached)
        self.cache = cache
        # stream: what is file-backed and not resident is decoded on the device (yogo_amd/image_stream.py); the items are the stream's,
        # in collate_cached's form, and the host loader is never iterated
        self.stream, self.normalize_images = stream, bool(normalize_images)
        self.dataset = loader.dataset if dataset is None else dataset
        self.sampler, self.batch_size = loader.sampler, loader.batch_size

    def __len__(self) -> int:
        return len(self.loader)

    def __iter__(self):
        dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        multi = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        if self.cache is not None:
            self.cache.prefill()   # once, before the split's first batch (and before its workers start)
        if self.cache is not None and self.cache.full:
            source = self._resident_batches()
        elif self.stream is not None:
            source = self.stream.batches([int(i) for i in iter(self.sampler)], self.batch_size)
        else:
            source = self.loader
        for item in source:
            if item is None:
                # every sample of the batch was unreadable (the robust collate of yogo/data/utils.py:49-63 returned nothing).  A
                # single process just skips it; under data parallelism a rank that skips a step issues one gradient all-reduce
                # fewer than its peers and the job hangs -- fail loudly instead
                if multi and self.strict_steps:
                    raise RuntimeError("yogo_amd: a whole batch of this rank was unreadable; in a data-parallel run every rank must "
                                       "take the same number of steps (fix or remove the unreadable files)")
                continue
            if self.cache is not None or self.stream is not None:
                imgs, labels = self._assemble_cached(item, dev)
            elif self.blob is not None:
                imgs, labels = self._assemble(item, dev)
            else:
                imgs, rows = item
                imgs = imgs.to(dev, non_blocking=True)
                labels = format_labels_batch(rows, self.Sx, self.Sy, "cxcywh", device=dev)
            yield self.transforms(imgs, labels)

    def _assemble(self, item, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        """a mixed batch on the device: real images uploaded into their rows, blob images composed into theirs, both label sets
        rasterised (one launch each) into their rows"""
        real_imgs, real_rows, real_pos, blob_idx, blob_pos, B = item
        blob = self.blob
        H, W = blob.background_img_shape
        with torch.cuda.device(dev):
            imgs = torch.empty(B, 1, H, W, dtype=torch.float32 if blob.normalize_images else torch.uint8, device=dev)
            labels = torch.empty(B, 6, self.Sy, self.Sx, dtype=torch.float32, device=dev)
            if real_pos:
                rp = torch.tensor(real_pos, dtype=torch.long).to(dev, non_blocking=True)
                imgs.index_copy_(0, rp, real_imgs.to(dev, non_blocking=True).to(imgs.dtype))
                labels.index_copy_(0, rp, format_labels_batch(real_rows, self.Sx, self.Sy, "cxcywh", device=dev))
            if blob_idx:
                _, blob_labels, _, _ = blob.generate(blob_idx, getattr(self.sampler, "epoch", 0), out_imgs=imgs, positions=blob_pos)
                labels.index_copy_(0, torch.tensor(blob_pos, dtype=torch.long).to(dev, non_blocking=True), blob_labels)
        return imgs, labels

    def _resident_batches(self):
        """the batches of a fully resident split in collate_cached's form, without the host DataLoader: the sampler's indices
        in chunks of batch_size (the DataLoader's boundaries, drop_last=False)"""
        order = [int(i) for i in iter(self.sampler)]
        for k in range(0, len(order), self.batch_size):
            chunk = order[k:k + self.batch_size]
            yield None, [], [], chunk, list(range(len(chunk))), [], [], len(chunk)

    def _assemble_cached(self, item, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        """a batch of a cached or streamed split on the device: uploaded rows with index_copy_ -- streamed rows (``Staged``) with a
        gather launch from their staging tensor instead --, resident rows with one gather launch, blob rows composed; the label rows
        of all real samples (uploaded or streamed, and resident, in batch order) rasterised by one launch"""
        up_imgs, up_rows, up_pos, res_idx, res_pos, blob_idx, blob_pos, B = item
        cache = self.cache
        C, H, W = cache.image_shape if cache is not None else self.stream.image_shape
        dtype = torch.float32 if (cache.normalize_images if cache is not None else self.normalize_images) else torch.uint8
        with torch.cuda.device(dev):
            imgs = torch.empty(B, C, H, W, dtype=dtype, device=dev)
            if up_pos and isinstance(up_imgs, Staged):
                slots = [-1] * B
                for p, s in zip(up_pos, up_imgs.slots):
                    slots[p] = s
                gather(up_imgs.images, slots, imgs)
            elif up_pos:
                imgs.index_copy_(0, torch.tensor(up_pos, dtype=torch.long).to(dev, non_blocking=True),
                                 up_imgs.to(dev, non_blocking=True).to(dtype))
            if res_pos:
                slots = [-1] * B
                for p, i in zip(res_pos, res_idx):
                    slots[p] = i
                gather(cache.images, slots, imgs)
            rows_at = dict(zip(up_pos, up_rows))
            rows_at.update((p, cache.label_rows(i)) for p, i in zip(res_pos, res_idx))
            real_pos = sorted(rows_at)
            real_labels = format_labels_batch([rows_at[p] for p in real_pos], self.Sx, self.Sy, "cxcywh", device=dev)
            if not blob_pos:
                return imgs, real_labels
            labels = torch.empty(B, 6, self.Sy, self.Sx, dtype=torch.float32, device=dev)
            if real_pos:
                labels.index_copy_(0, torch.tensor(real_pos, dtype=torch.long).to(dev, non_blocking=True), real_labels)
            _, blob_labels, _, _ = self.blob.generate(blob_idx, getattr(self.sampler, "epoch", 0), out_imgs=imgs, positions=blob_pos)
            labels.index_copy_(0, torch.tensor(blob_pos, dtype=torch.long).to(dev, non_blocking=True), blob_labels)
        return imgs, labels


def get_dataloader(dataset_definition: DatasetDefinition, batch_size: int, Sx: int, Sy: int, training: bool = True,
                   image_hw: Tuple[int, int] = (772, 1032), rgb: bool = False, normalize_images: bool = False,
                   split_fraction_override: Optional[SplitFractions] = None, device=None,
                   device_image_cache_gib: Optional[float] = None, device_image_decode: bool = False,
                   device_image_resize: bool = False, device_image_decode_all: bool = False, device_image_stream: bool = False,
                   stream_decode_batch: int = DEFAULT_DECODE_BATCH, device_image_decode_jpeg: bool = False) -> Dict[str, DeviceLoader]:
    """{split: DeviceLoader}.  device_image_cache_gib: keep decoded images of the train split, then of the val split with what
    is left, resident in HBM within this many GiB (yogo_amd/image_cache.py); None: no cache.  device_image_decode: fill that
    cache from PNG files inflated and unfiltered on the device (yogo_amd/png_prefill.py) instead of a pool of PIL workers.
    device_image_resize: on that route, resize the files of another size than image_hw on the device as well.
    device_image_decode_all: on that route, decode every PNG colour type, bit depth and Adam7 on the device, not 8-bit greyscale
    and RGB alone.
    device_image_decode_jpeg: on that route, decode baseline JPEG files (found by their first bytes) on the device as well
    (csrc/jpeg_decode.hip); progressive, CMYK, 12-bit and damaged ones stay on the host.
    device_image_stream: decode what is file-backed and not resident on the device too, every epoch, in groups of stream_decode_batch
    images, without DataLoader workers (yogo_amd/image_stream.py); it needs no cache.  device_image_resize and
    device_image_decode_all / device_image_decode_jpeg then widen what the stream decodes as well.  Its staging and scratch, shared by the splits, are allocated
    at the first iteration, are not part of the GIB budget, and are released by ``loader.stream.scratch.close()``."""
    if _stream_scope[0]:
        device_image_stream = True
        device_image_decode_all, device_image_resize = device_image_decode_all or _stream_scope[1], device_image_resize or _stream_scope[2]
        device_image_decode_jpeg = device_image_decode_jpeg or _stream_jpeg
    if device_image_decode and device_image_cache_gib is None:
        raise ValueError(f"{DECODE_FLAG} fills the device image cache: it needs {FLAG} GIB")
    if device_image_resize and not (device_image_decode or device_image_stream):
        raise ValueError(f"{RESIZE_FLAG} resizes what the device decoded: it needs {DECODE_FLAG}")
    if device_image_decode_all and not (device_image_decode or device_image_stream):
        raise ValueError(f"{DECODE_ALL_FLAG} widens what {DECODE_FLAG} takes: it needs {DECODE_FLAG}")
    if device_image_decode_jpeg and not (device_image_decode or device_image_stream):
        raise ValueError(f"{DECODE_JPEG_FLAG} widens what {DECODE_FLAG} takes: it needs {DECODE_FLAG}")
    budget = budget_bytes(device_image_cache_gib) if device_image_cache_gib is not None else None
    split_datasets = get_datasets(dataset_definition, Sx, Sy, rgb=rgb, image_hw=image_hw, normalize_images=normalize_images,
                                  split_fraction_override=split_fraction_override)
    augmentations = [RandomHorizontalFlipWithBBs(0.5), RandomVerticalFlipWithBBs(0.5)] if training else []
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank, world_size = torch.distributed.get_rank(), torch.distributed.get_world_size()
    else:
        rank, world_size = 0, 1
    # the budget covers the train split first, the val split gets what is left; the test split is read once and never cached
    image_shape = (3 if rgb else 1, int(image_hw[0]), int(image_hw[1]))
    resident: Dict[str, int] = {}
    for designation in ("train", "val"):
        if budget is not None and designation in split_datasets:
            resident[designation] = resident_count(budget, _real_len(split_datasets[designation]), *image_shape)
            budget -= resident[designation] * image_shape[0] * image_shape[1] * image_shape[2]
    stream_args = {}
    if device_image_stream:   # one scratch for every split: the threads of a rank are its share of the CPUs, as its workers would be
        stream_args = dict(scratch=Scratch(image_shape, batch_size, stream_decode_batch, device, bool(device_image_resize), bool(device_image_decode_all),
                                           max_threads=max(1, (guess_suggested_num_workers() or 1) // world_size),
                                           **({"decode_jpeg": True} if device_image_decode_jpeg else {})),
                           image_shape=image_shape, normalize_images=normalize_images, log=rank == 0)
    d: Dict[str, DeviceLoader] = {}
    for designation, dataset in split_datasets.items():
        if len(dataset) == 0:   # type: ignore[arg-type]
            continue
        augs = augmentations if designation == "train" else []
        cache_args = {}
        if resident.get(designation, 0) > 0:
            cache_args = dict(resident=resident[designation], image_shape=image_shape, normalize_images=normalize_images,
                              name=designation, log=rank == 0, device_decode=bool(device_image_decode),
                              device_resize=bool(device_image_resize and device_image_decode),
                              device_decode_all=bool(device_image_decode_all and device_image_decode),
                              device_decode_jpeg=bool(device_image_decode_jpeg and device_image_decode))
        if stream_args:
            cache_args = {**stream_args, "name": designation, **cache_args}
        d[designation] = _get_dataloader(dataset, batch_size, augs, rank, world_size, Sx, Sy, device, strict_steps=designation == "train",
                                         **cache_args)
    return d


def _real_len(dataset: Dataset) -> int:
    """the number of real (file-backed) samples of a split: all of it, less the BlobDataset of a thumbnail-augmented one"""
    if isinstance(dataset, ConcatDataset) and isinstance(dataset.datasets[-1], BlobDataset):
        return len(dataset) - len(dataset.datasets[-1])
    return len(dataset)   # type: ignore[arg-type]


def _num_workers(dataset_size: int, world_size: int) -> int:
    num_workers = choose_dataloader_num_workers(dataset_size) // world_size
    if dataset_size >= 1000:
        num_workers = max(1, num_workers)
    return num_workers


def _get_dataloader(dataset: Dataset, batch_size: int, augmentations: list, rank: int, world_size: int, Sx: int, Sy: int,
                    device=None, strict_steps: bool = False, resident: int = 0, image_shape: Optional[Tuple[int, int, int]] = None,
                    normalize_images: bool = False, name: str = "train", log: bool = False, device_decode: bool = False,
                    device_resize: bool = False, device_decode_all: bool = False, scratch: Optional[Scratch] = None,
                    device_decode_jpeg: bool = False) -> DeviceLoader:
    """resident > 0: split indices 0 .. resident-1 are kept decoded on the device (image_shape = (C, H, W)).  scratch: the split's
    file-backed samples that are not resident are streamed through it (yogo_amd/image_stream.py); no worker is ever started"""
    blob = dataset.datasets[-1] if isinstance(dataset, ConcatDataset) and isinstance(dataset.datasets[-1], BlobDataset) else None
    # the workers iterate the split with its blob part replaced by the indices alone (same length: same sampler order)
    host_dataset = ConcatDataset([*dataset.datasets[:-1], BlobIndices(len(blob))]) if blob is not None else dataset
    sampler: Iterable = DistributedSampler(host_dataset, rank=rank, num_replicas=world_size)   # torch defaults: shuffle, seed 0, padded
    num_workers = _num_workers(len(dataset), world_size)   # type: ignore[arg-type]
    cache = None
    collate_fn = collate_rows if blob is None else collate_mixed
    if resident > 0:
        # every rank keeps all indices < resident (DistributedSampler hands it different ones every epoch), prefilled by its own
        # workers; the split's workers see the resident indices as markers
        cache = ImageCache(dataset, resident, image_shape, normalize_images, device=device, num_workers=num_workers, batch_size=batch_size,
                           name=name, log=log, **({"device_decode": True} if device_decode else {}),
                           **({"device_resize": True} if device_resize else {}),
                           **({"device_decode_all": True} if device_decode_all else {}),
                           **({"device_decode_jpeg": True} if device_decode_jpeg else {}))   # (the keywords only when set:
        #                    tests/test_image_cache_host.py puts a recording class with the earlier signature in ImageCache's place)
        host_dataset = ResidentMarkers(host_dataset, cache.resident)
        collate_fn = collate_cached
    stream = None
    if scratch is not None:   # (the DataLoader below stays for dataset / sampler / batch_size / __len__ alone)
        stream = ImageStream(dataset, _real_len(dataset), scratch, cache=cache, name=name, log=log)
        num_workers = 0
    loader = DataLoader(host_dataset, shuffle=False, sampler=sampler, drop_last=False, pin_memory=torch.cuda.is_available(), batch_size=batch_size,
                        num_workers=num_workers, persistent_workers=num_workers > 0, generator=torch.Generator().manual_seed(SPLIT_SEED),
                        collate_fn=collate_fn, multiprocessing_context="spawn" if num_workers > 0 else None)
    return DeviceLoader(loader, Sx, Sy, MultiArgSequential(*augmentations), device, strict_steps=strict_steps, blob=blob,
                        dataset=dataset if blob is not None or cache is not None else None, cache=cache, stream=stream,
                        normalize_images=normalize_images)


def get_class_counts(d, num_classes: int, verbose: bool = True) -> torch.Tensor:
    """class histogram of the objects a loader yields (yogo_dataloader.py:284-311)"""
    class_counts = torch.zeros(num_classes, dtype=torch.long)
    for _, labels in d:
        bs, pd, Sy, Sx = labels.shape
        flat = labels.permute(1, 0, 2, 3).reshape(pd, bs * Sy * Sx)
        flat = flat[:, flat[0, :] == 1].long()
        class_counts += torch.bincount(flat[5, :], minlength=num_classes).cpu()
    return class_counts


def get_image_count(d) -> int:
    if isinstance(d.dataset, ConcatDataset):
        return d.dataset.cumulative_sizes[-1]
    if isinstance(d.dataset, Subset):
        return len(d.dataset)
    raise TypeError(f"unknown type {type(d.dataset)}")
