"""Labelled batches whose images are decoded on the device every epoch (``device_image_stream``, ``yogo train | test --device-image-stream``).

The device image cache (yogo_amd/image_cache.py) decodes a split once.  What it does not hold -- the test split, a val split the
budget did not reach, the train samples beyond ``resident_count``, everything when there is no cache -- DataLoader workers PIL-decode
again in every epoch.  This module takes the workers' place for those samples: no worker process is started; the sampler's order is
cut into the DataLoader's batches, consecutive batches are joined into decode GROUPS of at most ``decode_batch`` streamed samples
(``groups``), a group is decoded by one ``png_prefill.Filler.fill`` -- the prefill's routine, its host fallback, its resize and
decode-all routes -- into a staging tensor in HBM, and every batch of the group is gathered from there (``image_cache.gather``, the
launch that serves the cache's resident rows).  A group, not a batch, is the unit because a decode launch costs about the same for 256
streams as for 1 024 (README: the prefill's sweep).

A sample is STREAMED when it is file-backed and not resident: there is no cache, or its index lies beyond the cache, or it was
unreadable at the prefill.  Blob indices and resident indices pass through as they are.

Two staging tensors of ``max(decode_batch, batch_size)`` images: a loader thread fills group g + 1 on the filler's side stream while
the caller consumes group g (``device_decode.PrefetchFeed``).  A group is handed over behind an event, and its staging is filled again
only behind an event the caller's stream recorded after the last gather from it.  The staging, the filler and its scratch belong to
one ``Scratch`` that the splits of a ``get_dataloader`` call share: allocated at the first iteration, outside the cache's GIB budget,
released by ``close()``.  One iteration at a time uses them: starting one stops the thread of an iteration that was abandoned, and
that iteration raises if it is asked for more.

The batches are the worker route's, bit for bit (``--device-image-resize`` excepted, see png_prefill.py): a sample nothing can decode is
dropped and its batch closes up in the sampler's order, a batch with nothing left is the ``None`` item of the robust collate, a label
file that does not parse raises at the batch that holds it.  torch's global RNG is never drawn from, so the flips come out the same.
"""
from __future__ import annotations

import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
from torch.utils.data import Dataset

from yogo_amd.device_decode import MAX_THREADS, PrefetchFeed
from yogo_amd.image_cache import ImageCache, resolve_sample
from yogo_amd.png_prefill import DEFAULT_DECODE_BATCH, Filler, check_decode_batch

STREAM_FLAG = "--device-image-stream"


def groups(order: Sequence[int], batch_size: int, streamed: Callable[[int], bool], decode_batch: int = DEFAULT_DECODE_BATCH) -> List[List[List[int]]]:
    """The sampler's ``order`` cut into the DataLoader's batches (``batch_size`` at a time, the last one may be short) and those joined
    into decode groups: a group is a maximal run of consecutive whole batches whose streamed samples (``streamed(index)`` true) number
    at most ``decode_batch``.  A group holds at least one batch: a batch with more streamed samples than ``decode_batch`` is a group
    of its own.  -> groups of batches of indices; every batch once, in order."""
    batch_size, decode_batch = int(batch_size), check_decode_batch(decode_batch)
    if batch_size < 1:
        raise ValueError(f"groups: batch_size {batch_size} < 1")
    order = [int(i) for i in order]
    out: List[List[List[int]]] = []
    held = 0
    for lo in range(0, len(order), batch_size):
        batch = order[lo:lo + batch_size]
        n = sum(1 for i in batch if streamed(i))
        if out and held + n <= decode_batch:
            out[-1].append(batch)
            held += n
        else:
            out.append([batch])
            held = n
    return out


class Staged:
    """The streamed rows of one batch, where ``collate_cached`` has the stacked uploaded images: ``images[slots[k]]`` is the image of
    the batch's k-th streamed sample (uint8, on the device)."""

    def __init__(self, images: torch.Tensor, slots: List[int]):
        self.images, self.slots = images, slots


class Scratch:
    """What the streams of one ``get_dataloader`` call share: the ``Filler`` (pinned slots, stored streams, scanlines, thread pools, side
    stream) and the two staging tensors, made at the first iteration and kept until ``close()``; and which iteration uses them now."""

    def __init__(self, image_shape: Tuple[int, int, int], batch_size: int, decode_batch: int = DEFAULT_DECODE_BATCH, device=None,
                 device_resize: bool = False, decode_all: bool = False, max_threads: int = MAX_THREADS, decode_jpeg: bool = False):
        self.image_shape = tuple(int(v) for v in image_shape)
        self.decode_batch = check_decode_batch(decode_batch)
        self.capacity = max(self.decode_batch, int(batch_size))
        self.device, self.device_resize, self.decode_all, self.decode_jpeg = device, bool(device_resize), bool(decode_all), bool(decode_jpeg)
        self.max_threads = max(1, min(MAX_THREADS, int(max_threads)))
        self.filler: Optional[Filler] = None
        self.staging: List[torch.Tensor] = []
        self.released: List[Optional[torch.cuda.Event]] = [None, None]   # per staging tensor: after the caller's last gather from it
        self.active: Optional["_Iteration"] = None

    def open(self) -> torch.device:
        if not torch.cuda.is_available():
            raise RuntimeError(f"yogo_amd: {STREAM_FLAG} decodes images on an MI355X device; there is no CPU fallback")
        dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError(f"yogo_amd: {STREAM_FLAG} decodes images on an MI355X device (got {dev}); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self.filler is None:
            self.filler = Filler(dev, self.max_threads)
            try:
                self.staging = [torch.empty((self.capacity, *self.image_shape), dtype=torch.uint8, device=dev) for _ in range(2)]
            except RuntimeError as e:   # torch.OutOfMemoryError included
                self.filler = None
                raise RuntimeError(f"yogo_amd: {STREAM_FLAG}: could not allocate two staging tensors of {self.capacity} images on {dev}; "
                                   f"a smaller decode group needs less ({e})") from e
        return dev

    @property
    def hbm_bytes(self) -> int:
        return sum(t.numel() for t in self.staging) + (self.filler.device_bytes if self.filler is not None else 0)

    @property
    def pinned_bytes(self) -> int:
        return self.filler.pinned_bytes if self.filler is not None else 0

    def take(self, iteration: Optional["_Iteration"]) -> None:
        """`iteration` is the one that uses the scratch from here on: whichever did before is stopped first"""
        if self.active is not None and self.active is not iteration:
            self.active.stop()
        self.active = iteration

    def close(self) -> None:
        self.take(None)
        if self.filler is not None:
            self.filler.close()
            torch.cuda.synchronize(self.filler.device)   # (the caller's gathers have read the staging)
        self.filler, self.staging, self.released = None, [], [None, None]


class _Iteration(PrefetchFeed):
    """one pass over a split: item g is the list of group g's batches in ``collate_cached``'s form (``Staged`` for the images)"""

    def __init__(self, stream: "ImageStream", plan: List[List[List[int]]], dev: torch.device):
        super().__init__(len(plan), 1, "image-stream")
        self.stream, self.plan, self.dev = stream, plan, dev
        self.stopped = False

    def stop(self) -> None:
        self.stopped = True
        self.close()   # (waits for the group that is being filled)

    def close(self) -> None:
        super().close()
        if self.stream.scratch.active is self:
            self.stream.scratch.active = None

    def __next__(self):
        if self.stopped:
            raise RuntimeError(f"yogo_amd: {STREAM_FLAG}: this iteration was abandoned when another one started on the shared staging")
        n = self._pos
        if n < len(self.batches):
            # group n + 1 goes where group n - 1 was (group 0: where an earlier iteration's last group may have been): everything
            # that gathered from there is on the caller's stream by now
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.dev))
            self.stream.scratch.released[(n + 1) % 2] = ev
            if n == 0:
                self.stream.scratch.released[0] = ev
        try:
            return super().__next__()
        except StopIteration:
            raise
        except BaseException:
            self.close()
            raise

    def _load(self, g: int):
        """(loader thread) group g decoded into its staging tensor -> its batches, the event behind the side stream's work"""
        st, sc = self.stream, self.stream.scratch
        if self.stopped:
            return [], None
        real_len = st.real_len
        order = [i for batch in self.plan[g] for i in batch if st.streamed(i)]
        staging = sc.staging[g % 2]
        stats: Dict = {}
        t0 = time.perf_counter()
        with torch.cuda.device(self.dev):
            rows = sc.filler.fill(staging[:len(order)], [resolve_sample(st.dataset, i) for i in order], sc.decode_batch, stats,
                                  device_resize=sc.device_resize, decode_all=sc.decode_all, raise_rows=False, after=sc.released[g % 2],
                                  **({"decode_jpeg": True} if sc.decode_jpeg else {}))
            ev = torch.cuda.Event()
            ev.record(sc.filler.side)
        st._count(len(order), stats, time.perf_counter() - t0)
        items, slot = [], 0
        for batch in self.plan[g]:
            up_rows: List[torch.Tensor] = []
            up_pos: List[int] = []
            slots: List[int] = []
            res_idx: List[int] = []
            res_pos: List[int] = []
            blob_idx: List[int] = []
            blob_pos: List[int] = []
            error: Optional[BaseException] = None
            b = 0
            for i in batch:
                if i >= real_len:
                    blob_idx.append(i - real_len)
                    blob_pos.append(b)
                elif not st.streamed(i):
                    res_idx.append(i)
                    res_pos.append(b)
                else:
                    r, s = rows[slot], slot
                    slot += 1
                    if r is None:   # nothing could decode it: the batch closes up
                        continue
                    if isinstance(r, BaseException):
                        error = error or r
                        continue
                    up_rows.append(r)
                    up_pos.append(b)
                    slots.append(s)
                b += 1
            if error is not None:
                items.append(error)
            elif b == 0:
                items.append(None)
            else:
                items.append((Staged(staging, slots) if slots else None, up_rows, up_pos, res_idx, res_pos, blob_idx, blob_pos, b))
        return items, ev

    def _deliver(self, g: int, loaded):
        """(caller's thread) the group's batches behind the side stream's work"""
        items, ev = loaded
        if self.stopped or ev is None:
            raise RuntimeError(f"yogo_amd: {STREAM_FLAG}: this iteration was abandoned when another one started on the shared staging")
        with torch.cuda.device(self.dev):
            cur = torch.cuda.current_stream(self.dev)
            cur.wait_event(ev)
            self.stream.scratch.staging[g % 2].record_stream(cur)
        return items


class ImageStream:
    """The stream of one split.  dataset: the split as ``get_datasets`` made it (its blob part, if any, last); cache: its device image
    cache or None.  ``batches(order, batch_size)`` yields the split's batches in ``collate_cached``'s form, ``Staged`` in the images'
    place.  ``stats`` adds up over the iterations: ``groups``, ``streamed`` samples, ``host_decoded``, ``device_resized``, the
    per-chunk event times of ``fill`` (``inflate_ms``, ``unpack_ms``, ``resize_ms``; with the scratch's ``decode_jpeg`` also
    ``jpeg_decoded`` and ``jpeg_ms``), ``seconds`` spent filling, and the scratch's
    ``hbm_bytes`` / ``pinned_bytes`` as they stood after the last group."""

    def __init__(self, dataset: Dataset, real_len: int, scratch: Scratch, cache: Optional[ImageCache] = None, name: str = "train", log: bool = False):
        self.dataset, self.real_len, self.scratch, self.cache, self.name, self.log = dataset, int(real_len), scratch, cache, name, log
        self.image_shape, self.iterations = scratch.image_shape, 0
        self.stats: Dict = dict(groups=0, streamed=0, host_decoded=0, device_resized=0, inflate_ms=[], unpack_ms=[], resize_ms=[], seconds=0.0,
                                hbm_bytes=0, pinned_bytes=0)

    def streamed(self, i: int) -> bool:
        """file-backed and not resident"""
        if i >= self.real_len:
            return False
        cache = self.cache
        return cache is None or i >= cache.S or not cache.resident[i]

    def _count(self, n: int, stats: Dict, seconds: float) -> None:
        s = self.stats
        s["groups"] += 1
        s["streamed"] += n
        s["seconds"] += seconds
        for key in ("host_decoded", "device_resized"):
            s[key] += stats.get(key, 0)
        for key in ("inflate_ms", "unpack_ms", "resize_ms"):
            s[key].extend(stats.get(key, []))
        if "jpeg_ms" in stats:   # (--device-image-decode-jpeg)
            s["jpeg_decoded"] = s.get("jpeg_decoded", 0) + stats["jpeg_decoded"]
            s.setdefault("jpeg_ms", []).extend(stats["jpeg_ms"])
        s["hbm_bytes"], s["pinned_bytes"] = self.scratch.hbm_bytes, self.scratch.pinned_bytes

    def batches(self, order: Sequence[int], batch_size: int):
        dev = self.scratch.open()
        it = _Iteration(self, groups(order, batch_size, self.streamed, self.scratch.decode_batch), dev)
        self.scratch.take(it)
        before = {k: self.stats[k] for k in ("groups", "streamed", "seconds", "host_decoded", "device_resized")}
        try:
            for items in it:
                for item in items:
                    if it.stopped:   # (the rest of this group's staging belongs to another iteration now)
                        raise RuntimeError(f"yogo_amd: {STREAM_FLAG}: this iteration was abandoned when another one started on the shared staging")
                    if isinstance(item, BaseException):
                        raise item
                    yield item
        finally:
            it.close()
        self.iterations += 1
        if self.log and self.iterations == 1:
            s = self.stats
            n, dt = s["streamed"] - before["streamed"], s["seconds"] - before["seconds"]
            print(f"yogo_amd: device image stream ({self.name}): {n} images in {s['groups'] - before['groups']} groups, "
                  f"{s['host_decoded'] - before['host_decoded']} decoded on the host, {s['device_resized'] - before['device_resized']} resized "
                  f"on the device; {n / max(dt, 1e-9):.0f} images/s decoding; {s['hbm_bytes']} bytes of HBM, {s['pinned_bytes']} pinned",
                  flush=True)
