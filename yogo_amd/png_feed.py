"""Inference batches from a directory of PNG files, decoded on the device (``yogo infer --path-to-images --device-image-decode``).

The reference's DataLoader workers decode every file with torchvision / PIL on the host.  Here a ``PngDeviceFeed`` takes the
DataLoader's place, a yogo_amd/device_decode.py PrefetchFeed as ZarrDeviceFeed is: per batch a thread pool reads the files and parses their
chunks (yogo_amd/png.py: signature, IHDR, CRC-32 of IHDR and of every IDAT chunk), the IDAT payloads of a file are copied back to
back into a pinned buffer -- one zlib stream per image -- and go up on a side stream as they came off the disk;
``yogo_inflate_zlib`` (csrc/inflate.hip) inflates every image's scanlines, one wavefront each, and ``yogo_png_unpack``
(csrc/png_unpack.hip, the loop of csrc/png_unfilter.h) reverses the PNG filters, crops and optionally divides by 255 into the
batch.  Two slots: the loader thread reads and decodes batch n+1 while the caller works on batch n.  What lies between a file's
bytes and the unpack launch -- the record of a file, the layout of the scanline buffer, the inflate launch, the unpack table -- is
yogo_amd/png_batch.py's, shared with the prefill of the device image cache (yogo_amd/png_prefill.py); what is the feed's own is here:
which files it accepts, how the pinned slots are sized, and what a failure means.  Every image has its own place in the scanline
buffer, at what its stream inflates to; a slot gives every image the same room, sized from the longest stream of the first batch.

What the device does not take -- anything but 8-bit greyscale without interlace or transparency, a file that does not parse as PNG,
a file larger than the room a slot has per image -- is decoded by ``read_image`` on the host and enters the unpack launch as a raw
image.  A file nothing can decode, or whose size differs from the first file's of its batch, raises RuntimeError naming it and
costs exactly its batch, the class ``predict`` warns on and goes on.

``all_types=True`` (``--device-image-decode-all``) sends every parsable PNG to the device instead: all colour types and bit depths,
tRNS or not, Adam7 (``PngInfo.any_decodable``), unpacked by ``yogo_png_unpack_any`` (csrc/png_unpack_any.hip, the same loop) into
1 plane or, for an RGB model (``rgb=True``), 3, converted as ``read_image(path, rgb)`` converts them.  The images of a batch may
each be of another format: the palettes of the batch's palette files lie behind the last image of the scanline buffer, and the
pinned slot gives every file room for its own size.  Still one inflate and one unpack launch per batch; the host keeps another
format under a .png name, a stream larger than its room and a palette file without a usable PLTE chunk.

``jpeg=True`` (``--device-image-decode-jpeg``) has the device take a baseline JPEG file found in the directory as well
(``JpegInfo.device_decodable``; the reference globs ``*.png`` alone, so it is a file under the wrong name: it is taken by its first
bytes): its bytes go into its room as they are, ONE ``yogo_jpeg_decode`` launch per batch that has such files (csrc/jpeg_decode.hip)
leaves their planes in the scanline buffer, and the batch's unpack launch takes them as raw images.  A file the kernel gives a
status is decoded by ``read_image`` after all and the batch is unpacked again.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Tuple

import numpy as np
import torch

from yogo_amd import inflate, png
from yogo_amd.device_decode import ALIGN, MAX_THREADS, PrefetchFeed, center_crop_origin, feed_device, gather, png_unpack, png_unpack_any, \
    raise_first_bad
from yogo_amd.png_batch import PngStream, Refused, _file_size, batch_layout, inflate_batch, jpeg_batch, read_jpeg_stream, read_stream, slot_layout, \
    unpack_table, upload_host_parts
from yogo_amd.yogo_dataset import read_image

UNPACK_STATUS = {1: "a filter-type byte above 4", 2: "the image lies outside the scanline buffer"}


class PngDeviceFeed(PrefetchFeed):
    """Iterator over ``(device batch [B, 1, OH, OW], tuple of paths)`` in the dataset's order; the last batch may be partial; a batch
    that raises RuntimeError costs that batch alone (device_decode.PrefetchFeed).  ``crop``: (OH, OW) of a centre crop done in the
    kernel; ``normalize``: fp32 ``/ 255`` in the kernel, else uint8.  ``all_types``: every PNG colour type, bit depth and Adam7 goes
    to the device (see the module's text); ``rgb`` (with all_types only): batches of 3 planes, ``[B, 3, OH, OW]``; ``jpeg``: baseline
    JPEG files go to the device too (``jpeg_decoded`` counts them)."""

    all_types = rgb = jpeg = False   # (the defaults, also of an object made without __init__)

    def __init__(self, dataset, batch_size: int, device, crop: Optional[Tuple[int, int]] = None, normalize: bool = False,
                 all_types: bool = False, rgb: bool = False, jpeg: bool = False):
        dev = feed_device(device, batch_size, "the PNG feed decodes")
        if rgb and not all_types:
            raise ValueError("PngDeviceFeed: batches of 3 planes (rgb) need all_types: yogo_png_unpack writes one plane of 8-bit greyscale")
        self.dataset, self.batch_size, self.device, self.normalize = dataset, int(batch_size), dev, bool(normalize)
        self.all_types, self.rgb, self.jpeg = bool(all_types), bool(rgb), bool(jpeg)
        self.jpeg_decoded = 0   # images yogo_jpeg_decode served
        self._unpack = png_unpack_any if self.all_types else png_unpack
        self.crop = None if crop is None else (int(crop[0]), int(crop[1]))
        self.paths = [str(p) for p in dataset.image_paths]
        n = len(self.paths)
        self.room = 0   # (not all_types) bytes a slot has per image for its stored zlib stream; sized from the first batch
        self._pinned: List[Optional[torch.Tensor]] = [None, None]
        self._sdev: List[Optional[torch.Tensor]] = [None, None]
        self._scan: List[Optional[torch.Tensor]] = [None, None]
        self._side = torch.cuda.Stream(dev)
        self._pool = ThreadPoolExecutor(max_workers=max(1, min(MAX_THREADS, os.cpu_count() or 1)), thread_name_prefix="png-read")
        self.host_decoded = 0   # images that went through read_image
        super().__init__(n, self.batch_size, "png-feed")

    def close(self) -> None:
        super().close()
        self._pool.shutdown(wait=True)

    def _accept(self, info: png.PngInfo) -> bool:
        """what the unpack kernel of this feed takes"""
        return info.any_decodable if self.all_types else info.device_decodable

    def _host_image(self, path: str) -> PngStream:
        try:
            t = read_image(path, rgb=self.rgb)
        except Exception as e:
            raise RuntimeError(f"{path} could not be decoded ({type(e).__name__}: {e})") from e
        return PngStream((int(t.shape[1]), int(t.shape[2])), host=True, pixels=(t if self.rgb else t[0]).contiguous().numpy())

    def _read(self, path: str, room: Optional[np.ndarray]) -> PngStream:
        """(pool thread) one file: its zlib stream into ``room`` (this image's bytes of the slot's pinned buffer; None while the
        room is being sized: then the record keeps the stream itself), or its pixels from the host decoder"""
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError as e:
            raise RuntimeError(f"{path} could not be read ({type(e).__name__}: {e})") from e
        try:
            try:
                return read_stream(data, room, self._accept)
            except png.NotPng:
                if not self.jpeg:
                    raise
                try:
                    return read_jpeg_stream(data, room, lambda info: info.device_decodable, 3 if self.rgb else 1)
                except ValueError:   # (no JPEG either, one the kernel does not take or that does not parse: PIL's to read if it can)
                    return self._host_image(path)
        except (png.NotPng, Refused):   # another format under a .png name (PIL's to read if it can), a PNG this feed's kernel
            return self._host_image(path)   # does not take, a stream longer than its room
        except ValueError as e:
            raise RuntimeError(f"{path} could not be decoded ({e})") from e

    def _grow_slot(self, slot: int, nbytes: int) -> None:
        self._pinned[slot] = self._sdev[slot] = None   # (the smaller buffers go back first)
        self._pinned[slot] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self._sdev[slot] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def _read_batch(self, slot: int, paths: List[str]) -> Tuple[List[PngStream], np.ndarray]:
        """the files of a batch into the slot's pinned buffer -> (their records, where each one's room starts).  Where the rooms
        come from is the one thing the two modes do not share."""
        B = len(paths)
        if self.all_types:
            # the formats of a directory differ in size by more than an order of magnitude: every file has room for its own bytes
            # (an IDAT payload is shorter than its file), the slots grow with the largest batch
            sizes = list(self._pool.map(_file_size, paths))
            src_at, slot_bytes = slot_layout(sizes)
            if self._pinned[slot] is None or self._pinned[slot].numel() < slot_bytes:
                self._grow_slot(slot, -(-max(1, slot_bytes) * self.batch_size // B))
        elif self.room == 0:
            # the first batch sizes the slots -- the room per image from its longest stream, with a quarter and 4 KiB to spare --:
            # its streams come back as bytes and are copied in here
            images = gather([self._pool.submit(self._read, p, None) for p in paths])
            self.room = -(-(max((im.stored for im in images), default=0) * 5 // 4 + 4096) // ALIGN) * ALIGN
            for s in range(2):
                self._grow_slot(s, self.batch_size * self.room)
            host = self._pinned[slot].numpy()
            for i, im in enumerate(images):
                if im.stream is not None:
                    host[i * self.room:i * self.room + im.stored] = np.frombuffer(im.stream, dtype=np.uint8)
                    im.stream = None
            return images, np.arange(B, dtype=np.int64) * self.room
        else:
            src_at, sizes = np.arange(B, dtype=np.int64) * self.room, [self.room] * B
        host = self._pinned[slot].numpy()
        return gather([self._pool.submit(self._read, p, host[int(src_at[i]):int(src_at[i]) + sizes[i]]) for i, p in enumerate(paths)]), src_at

    def _load(self, n: int):
        """(loader thread) batch n: read, upload, inflate and unpack on the side stream, then the per-image status back"""
        slot = n % 2
        lo, hi = self.batches[n]
        paths = self.paths[lo:hi]
        B = len(paths)
        images, src_at = self._read_batch(slot, paths)
        H, W = images[0].hw
        for p, im in zip(paths, images):
            if im.hw != (H, W):
                raise RuntimeError(f"{p} is {im.hw[0]} x {im.hw[1]}, the first image of its batch ({paths[0]}) {H} x {W}")
        OH, OW = (H, W) if self.crop is None else self.crop
        try:
            top, left = center_crop_origin(H, W, OH, OW)
        except ValueError as e:
            raise RuntimeError(f"{paths[0]}: {e}") from e
        C = 3 if self.rgb else 1
        # every image at its own inflated size; behind the last one the palettes of the batch, 768 bytes each
        layout = batch_layout(images, C * H * W)
        if self._scan[slot] is None or self._scan[slot].numel() < layout.total:
            self._scan[slot] = None   # (the smaller buffer goes back to the allocator first)
            self._scan[slot] = torch.empty(-(-layout.total * self.batch_size // B), dtype=torch.uint8, device=self.device)
        scan = self._scan[slot]
        with torch.cuda.device(self.device), torch.cuda.stream(self._side):
            inflate_status, device_rows = inflate_batch(images, src_at, layout, self._pinned[slot], self._sdev[slot], scan)
            jpeg_status, jpeg_rows = jpeg_batch(images, src_at, layout, self._sdev[slot], scan, C)
            self.host_decoded += B - len(device_rows) - len(jpeg_rows)
            upload_host_parts(images, layout, scan)
            out = torch.empty((B, C, OH, OW), dtype=torch.float32 if self.normalize else torch.uint8, device=self.device)
            status = torch.empty(B, dtype=torch.int32, device=self.device)
            table = unpack_table(self._unpack, images, layout)
            self._unpack(scan, torch.from_numpy(table).to(self.device), (H, W), out, status, top, left)
            ev = torch.cuda.Event()
            ev.record(self._side)
            bad_inflate = inflate_status.cpu() if inflate_status is not None else None   # waits for the launches
            bad = status.cpu()
            refused = [] if jpeg_status is None else [jpeg_rows[k] for k in torch.nonzero(jpeg_status.cpu()).reshape(-1).tolist()]
            self.jpeg_decoded += len(jpeg_rows) - len(refused)
            if refused:   # what the JPEG kernel handed back: the host decoder's pixels in their place, and the batch unpacked again
                for i in refused:
                    images[i] = self._host_image(paths[i])
                    if images[i].hw != (H, W):
                        raise RuntimeError(f"{paths[i]} is {images[i].hw[0]} x {images[i].hw[1]}, the first image of its batch ({paths[0]}) {H} x {W}")
                    scan[int(layout.at[i]):int(layout.at[i]) + layout.need[i]].copy_(torch.as_tensor(images[i].pixels).contiguous().reshape(-1))
                self.host_decoded += len(refused)
                self._unpack(scan, torch.from_numpy(unpack_table(self._unpack, images, layout)).to(self.device), (H, W), out, status, top, left)
                ev.record(self._side)
                bad = status.cpu()
        raise_first_bad(bad_inflate, inflate.INF_STATUS, lambda row: paths[device_rows[row]])
        raise_first_bad(bad, UNPACK_STATUS, lambda row: paths[row])
        return out, tuple(paths), ev

    def _deliver(self, n: int, loaded) -> Tuple[torch.Tensor, Tuple[str, ...]]:
        """(caller's thread) the batch behind the side stream's work"""
        out, paths, ev = loaded
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            out.record_stream(cur)
        return out, paths
