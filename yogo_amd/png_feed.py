"""Inference batches from a directory of PNG files, decoded on the device (``yogo infer --path-to-images --device-image-decode``).

The reference's DataLoader workers decode every file with torchvision / PIL on the host.  Here a ``PngDeviceFeed`` takes the
DataLoader's place, a yogo_amd/device_decode.py PrefetchFeed as ZarrDeviceFeed is: per batch a thread pool reads the files and parses their
chunks (yogo_amd/png.py: signature, IHDR, CRC-32 of IHDR and of every IDAT chunk), the IDAT payloads of a file are copied back to
back into a pinned buffer -- one zlib stream per image -- and go up on a side stream as they came off the disk;
``yogo_inflate_zlib`` (csrc/inflate.hip) inflates every image's scanlines, one wavefront each, and ``yogo_png_unpack``
(csrc/png_unpack.hip, the loop of csrc/png_unfilter.h) reverses the PNG filters, crops and optionally divides by 255 into the
batch.  Two slots: the loader thread reads and decodes batch n+1 while the caller works on batch n.

What the device does not take -- anything but 8-bit greyscale without interlace or transparency, a file that does not parse as PNG,
a file larger than the room a slot has per image -- is decoded by ``read_image`` on the host and enters the unpack launch as a raw
image.  A file nothing can decode, or whose size differs from the first file's of its batch, raises RuntimeError naming it and
costs exactly its batch, the class ``predict`` warns on and goes on.

``all_types=True`` (``--device-image-decode-all``) sends every parsable PNG to the device instead: all colour types and bit depths,
tRNS or not, Adam7 (``PngInfo.any_decodable``), unpacked by ``yogo_png_unpack_any`` (csrc/png_unpack_any.hip, the same loop) into
1 plane or, for an RGB model (``rgb=True``), 3, converted as ``read_image(path, rgb)`` converts them.  The images of a batch may
each be of another format: every image has its own inflated size in the scanline buffer, the palettes of the batch's palette
files lie behind the last image; the pinned slot gives every file room for its own size.  Still one inflate and one unpack launch per batch; the host keeps another format under a .png
name, a stream larger than its room and a palette file without a usable PLTE chunk.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Tuple

import numpy as np
import torch

from yogo_amd import inflate, png
from yogo_amd.device_decode import ALIGN, MAX_THREADS, PrefetchFeed, center_crop_origin, gather, inflate_streams, png_stream_into, \
    png_unpack, png_unpack_any, raise_first_bad
from yogo_amd.png_prefill import slot_layout
from yogo_amd.yogo_dataset import read_image

UNPACK_STATUS = {1: "a filter-type byte above 4", 2: "the image lies outside the scanline buffer"}
SCAN_ALIGN = 16   # yogo_inflate_zlib asks for 16-byte aligned destinations


def _file_size(path: str) -> int:
    try:
        return os.stat(path).st_size
    except OSError:
        return 0


class _Image:
    """what one file of a batch turned out to be: a zlib stream for the device (``stored`` bytes at its place in the slot, the
    DEFLATE range and Adler-32 inside them; ``stream``: the bytes themselves while the slots are not sized yet) or pixels decoded
    on the host (``pixels``).  With all_types: ``need`` bytes the stream inflates to, the format ``code`` of yogo_png_unpack_any's
    table, the ``palette`` (768 bytes) of a palette file"""
    __slots__ = ("hw", "stored", "deflate", "adler", "pixels", "stream", "need", "code", "palette")

    def __init__(self, hw, stored=0, deflate=(0, 0), adler=0, pixels=None, stream=None, need=0, code=png.FMT_PLANAR, palette=None):
        self.hw, self.stored, self.deflate, self.adler, self.pixels, self.stream = hw, stored, deflate, adler, pixels, stream
        self.need, self.code, self.palette = need, code, palette


class PngDeviceFeed(PrefetchFeed):
    """Iterator over ``(device batch [B, 1, OH, OW], tuple of paths)`` in the dataset's order; the last batch may be partial; a batch
    that raises RuntimeError costs that batch alone (device_decode.PrefetchFeed).  ``crop``: (OH, OW) of a centre crop done in the
    kernel; ``normalize``: fp32 ``/ 255`` in the kernel, else uint8.  ``all_types``: every PNG colour type, bit depth and Adam7 goes
    to the device (see the module's text); ``rgb`` (with all_types only): batches of 3 planes, ``[B, 3, OH, OW]``."""

    all_types = rgb = False   # (the defaults, also of an object made without __init__)

    def __init__(self, dataset, batch_size: int, device, crop: Optional[Tuple[int, int]] = None, normalize: bool = False,
                 all_types: bool = False, rgb: bool = False):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"yogo_amd: the PNG feed decodes on an MI355X device (got {dev}); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if batch_size < 1 or batch_size > 65535:
            raise ValueError(f"batch size {batch_size} outside [1, 65535]")
        if rgb and not all_types:
            raise ValueError("PngDeviceFeed: batches of 3 planes (rgb) need all_types: yogo_png_unpack writes one plane of 8-bit greyscale")
        self.dataset, self.batch_size, self.device, self.normalize = dataset, int(batch_size), dev, bool(normalize)
        self.all_types, self.rgb = bool(all_types), bool(rgb)
        self.crop = None if crop is None else (int(crop[0]), int(crop[1]))
        self.paths = [str(p) for p in dataset.image_paths]
        n = len(self.paths)
        self.room = 0   # bytes a slot has per image for its stored zlib stream; sized from the first batch
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

    def _host_image(self, path: str) -> _Image:
        try:
            t = read_image(path, rgb=self.rgb)
        except Exception as e:
            raise RuntimeError(f"{path} could not be decoded ({type(e).__name__}: {e})") from e
        return _Image((int(t.shape[1]), int(t.shape[2])), pixels=(t if self.rgb else t[0]).contiguous().numpy())

    def _read(self, path: str, room: Optional[np.ndarray]) -> _Image:
        """(pool thread) one file: its zlib stream into ``room`` (this image's bytes of the slot's pinned buffer; None while the
        room is being sized: then the stream itself is returned), or its pixels from the host decoder"""
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError as e:
            raise RuntimeError(f"{path} could not be read ({type(e).__name__}: {e})") from e
        try:
            info = png.parse_png(data)
        except png.NotPng:
            return self._host_image(path)   # another format under a .png name: PIL's to read if it can
        except ValueError as e:
            raise RuntimeError(f"{path} could not be decoded ({e})") from e
        if not (info.any_decodable if self.all_types else info.device_decodable) or (room is not None and info.idat_bytes > len(room)):
            return self._host_image(path)
        stream = None
        try:
            if room is None:
                stream = b"".join(data[o:o + n] for o, n in info.idat)
                stored, (off, ln, adler) = len(stream), inflate.split_zlib(stream)
            else:
                stored, off, ln, adler = png_stream_into(data, info, room)
        except ValueError as e:
            raise RuntimeError(f"{path} could not be decoded ({e})") from e
        if not self.all_types:
            return _Image((info.height, info.width), stored, (off, ln), adler, stream=stream)
        return _Image((info.height, info.width), stored, (off, ln), adler, stream=stream, need=info.inflated_bytes, code=info.format_code,
                      palette=png.palette_table(data, info) if info.color_type == 3 else None)

    def _size_slots(self, streams: List[int], B: int) -> None:
        """the room per image from the longest stream of the first batch, with a quarter and 4 KiB to spare"""
        self.room = -(-(max(streams, default=0) * 5 // 4 + 4096) // ALIGN) * ALIGN
        for s in range(2):
            self._pinned[s] = torch.empty(B * self.room, dtype=torch.uint8).pin_memory()
            self._sdev[s] = torch.empty(B * self.room, dtype=torch.uint8, device=self.device)

    def _load(self, n: int):
        """(loader thread) batch n: read, upload, inflate and unpack on the side stream, then the per-image status back"""
        slot = n % 2
        lo, hi = self.batches[n]
        paths = self.paths[lo:hi]
        B = len(paths)
        if self.all_types:
            # the formats of a directory differ in size by more than an order of magnitude: every file has room for its own bytes
            # (an IDAT payload is shorter than its file), the slots grow with the largest batch
            sizes = list(self._pool.map(_file_size, paths))
            src_at, slot_bytes = slot_layout(sizes)
            if self._pinned[slot] is None or self._pinned[slot].numel() < slot_bytes:
                self._pinned[slot] = self._sdev[slot] = None   # (the smaller buffers go back first)
                grown = -(-max(1, slot_bytes) * self.batch_size // B)
                self._pinned[slot] = torch.empty(grown, dtype=torch.uint8).pin_memory()
                self._sdev[slot] = torch.empty(grown, dtype=torch.uint8, device=self.device)
            host = self._pinned[slot].numpy()
            images = gather([self._pool.submit(self._read, p, host[int(src_at[i]):int(src_at[i]) + sizes[i]]) for i, p in enumerate(paths)])
        elif self.room == 0:
            # the first batch sizes the slots: its streams come back as bytes and are copied in here
            images = gather([self._pool.submit(self._read, p, None) for p in paths])
            self._size_slots([im.stored for im in images], self.batch_size)
            host = self._pinned[slot].numpy()
            for i, im in enumerate(images):
                if im.stream is not None:
                    host[i * self.room:i * self.room + im.stored] = np.frombuffer(im.stream, dtype=np.uint8)
                    im.stream = None
        else:
            host = self._pinned[slot].numpy()
            images = gather([self._pool.submit(self._read, p, host[i * self.room:(i + 1) * self.room]) for i, p in enumerate(paths)])
        if not self.all_types:
            src_at = np.arange(B, dtype=np.int64) * self.room
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
        if self.all_types:
            # every image at its own inflated size; behind the last one the palettes of the batch, 768 bytes each
            need = [C * H * W if im.pixels is not None else im.need for im in images]
            at = np.zeros(B + 1, dtype=np.int64)
            at[1:] = np.cumsum([-(-v // SCAN_ALIGN) * SCAN_ALIGN for v in need])
            with_palette = [i for i, im in enumerate(images) if im.palette is not None]
            palette_at = {i: int(at[B]) + k * png.PALETTE_BYTES for k, i in enumerate(with_palette)}
            total = int(at[B]) + len(with_palette) * png.PALETTE_BYTES
            if self._scan[slot] is None or self._scan[slot].numel() < total:
                self._scan[slot] = None   # (the smaller buffer goes back to the allocator first)
                self._scan[slot] = torch.empty(-(-total * self.batch_size // B), dtype=torch.uint8, device=self.device)
            table = np.asarray([(int(at[i]), im.code, palette_at.get(i, 0)) for i, im in enumerate(images)], dtype=np.int64).reshape(-1, 3)
        else:
            stride = -(-(H * (1 + W)) // 16) * 16
            need, at = [H * W if im.pixels is not None else H * (1 + W) for im in images], np.arange(B + 1, dtype=np.int64) * stride
            if self._scan[slot] is None or self._scan[slot].numel() < B * stride:
                self._scan[slot] = torch.empty(self.batch_size * stride, dtype=torch.uint8, device=self.device)
            table = np.asarray([(i * stride, 0 if im.pixels is None else 1) for i, im in enumerate(images)], dtype=np.int64)
        scan = self._scan[slot]
        device_rows = [i for i, im in enumerate(images) if im.pixels is None]
        self.host_decoded += B - len(device_rows)
        rows = np.asarray([(int(src_at[i]) + images[i].deflate[0], images[i].deflate[1], int(at[i]), need[i], images[i].adler)
                           for i in device_rows], dtype=np.int64).reshape(-1, 5)
        with torch.cuda.device(self.device), torch.cuda.stream(self._side):
            inflate_status = None
            if device_rows:
                used = int(src_at[device_rows[-1]]) + images[device_rows[-1]].stored
                self._sdev[slot][:used].copy_(self._pinned[slot][:used], non_blocking=True)
                inflate_status = torch.empty(len(device_rows), dtype=torch.int32, device=self.device)
                inflate_streams(self._sdev[slot], torch.from_numpy(rows).to(self.device), scan, inflate_status)
            for i, im in enumerate(images):
                if im.pixels is not None:   # (rare: a pageable copy per image)
                    scan[int(at[i]):int(at[i]) + need[i]].copy_(torch.from_numpy(im.pixels).reshape(-1))
            out = torch.empty((B, C, OH, OW), dtype=torch.float32 if self.normalize else torch.uint8, device=self.device)
            status = torch.empty(B, dtype=torch.int32, device=self.device)
            if self.all_types:
                if with_palette:   # one copy for the palettes of the batch
                    palettes = torch.from_numpy(np.concatenate([images[i].palette for i in with_palette]))
                    scan[int(at[B]):total].copy_(palettes)
                png_unpack_any(scan, torch.from_numpy(table).to(self.device), (H, W), out, status, top, left)
            else:
                png_unpack(scan, torch.from_numpy(table).to(self.device), (H, W), out, status, top, left)
            ev = torch.cuda.Event()
            ev.record(self._side)
            bad_inflate = inflate_status.cpu() if inflate_status is not None else None   # waits for the launches
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
