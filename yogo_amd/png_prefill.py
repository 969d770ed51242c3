"""The device image cache filled from PNG files decoded on the device (``yogo train --device-image-cache GIB --device-image-decode``).

``ImageCache.prefill`` PIL-decodes the resident set once in a one-off pool of DataLoader workers.  ``fill`` here takes its place:
no worker processes, a pool of threads that only READ.  The N samples go in chunks of ``decode_batch``; per chunk the threads read
and parse every file (yogo_amd/png.py), copy its IDAT payloads back to back -- one zlib stream per image -- into a pinned slot and
parse the sample's label rows; then, on a side stream: the slot goes up, ONE ``yogo_inflate_zlib`` launch (csrc/inflate.hip, one
wavefront per stream) inflates every image's scanlines, ONE ``yogo_png_unpack_planes`` launch (csrc/png_unpack_planes.hip on csrc/png_unfilter.h) reverses
the filters and writes the planes straight into ``images[lo:hi]``, and the per-image statuses come back.  Two pinned slots: chunk
n + 1 is read while chunk n decodes.  The chunk is independent of the training batch, so thousands of streams share a launch.
The record of a file, the layouts of the slot and of the scanline buffer, the inflate launch and the unpack tables are
yogo_amd/png_batch.py's, shared with the inference feed (yogo_amd/png_feed.py); what is the prefill's own is here: which files it
accepts, the label rows, the resize groups, and the host decoder behind everything the device does not take or refuses.

A slot is sized from the files' sizes, known by ``stat`` before anything is read (an IDAT payload is shorter than its file): every
file has room at a multiple of ``ALIGN``, whatever the sizes of the files before it.

What the device takes: 8-bit greyscale and 8-bit RGB, not interlaced, no tRNS, of exactly ``image_hw``; the kernel converts to the
cache's channel count as ``read_image(path, rgb)`` does.  Everything else goes through ``ds.image_uint8(j)`` (PIL, its retries,
``resize_image``) and enters the unpack launch as planar pixels (kind 1): other bit depths and colour types, interlace, tRNS, a
file that is not a PNG under its name or does not parse, a file of another size than ``image_hw``, and a file whose inflate or unpack
status is not 0.  If that returns None the sample is not made resident, exactly as on the host route.

One divergence: a file that PIL rejects but this route accepts (a defect in a chunk that only PIL checks) is resident here and
not on the host route, where it stays with the workers.  Files both accept give the same bytes.

The scratch -- two pinned slots, the stored streams and the scanlines on the device -- belongs to a ``Filler``; ``fill`` makes one
for the call, so that there it lives only while ``fill`` runs (the per-epoch stream of yogo_amd/image_stream.py keeps one), and is NOT
part of the cache budget: per chunk the files' bytes twice pinned, once on the device, and what its stream inflates to
(``PngInfo.inflated_bytes``) of scanlines per image (``stats["scratch_device_bytes"]``, ``stats["scratch_pinned_bytes"]``).  torch's global RNG is not touched.

``device_resize=True`` (``--device-image-resize``) keeps a device-decodable file of ANOTHER size on the device as well, as long as
each axis scales down by at most ``resize.MAX_DOWNSCALE`` (up by anything): the files of a chunk are grouped by their size, a group is
inflated with the rest, unpacked by a ``yogo_png_unpack_planes`` launch of its own into a staging tensor ``[n, C, Hs, Ws]`` -- the
colour conversion comes before the resize, as in ``read_image`` then ``resize_image`` -- and ONE ``yogo_resize_aa_u8`` launch
(csrc/resize_aa.hip, the taps of yogo_amd/resize.py) writes it into the group's slots.  The staging is scratch like the rest.  The
pixels are those of the definition ``resize_image`` implements, computed in fp32 from fp64 taps; torch's CPU kernel rounds its own
way, so a few pixels per image whose exact value lies within about 1e-3 of a rounding edge may differ by one grey level from the
host route's.  Off (the default), nothing changes.

``decode_all=True`` (``--device-image-decode-all``) widens what the device takes to every PNG colour type and bit depth, tRNS or
not, Adam7-interlaced or not (``PngInfo.any_decodable``): the chunk's launch -- and with ``device_resize`` every group's -- is then
``yogo_png_unpack_any`` (csrc/png_unpack_any.hip, the same loop), whose table names each image's format, so one launch still takes
a chunk of mixed files; every image has its own inflated size in the scanline buffer and the palettes of the chunk's palette files
lie behind the last image.  The conversions are ``read_image``'s, bit for bit.  The host keeps what is no PNG, what does not parse,
a palette file without a usable PLTE chunk, and whatever the inflate or unpack launch refuses.  Off (the default), nothing changes.

``decode_jpeg=True`` (``--device-image-decode-jpeg``) has the device take baseline JPEG files too, by their first bytes and not their
name (``JpegInfo.device_decodable``: Huffman sequential, 8 bits, one scan, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, at most
``jpeg.MAX_WIDTH`` wide): the file's bytes go into its room of the slot as they are, ONE ``yogo_jpeg_decode`` launch per chunk
(csrc/jpeg_decode.hip) leaves every JPEG's planes in the scanline buffer where host-decoded pixels would lie, and the chunk's one
unpack launch takes them as planar entries beside the PNG files.  A JPEG of another size follows the ``device_resize`` rule of a PNG.
The host keeps progressive, arithmetic, 12-bit, CMYK, multi-scan and wider files and whatever the kernel gives a status
(``jpeg.JPG_STATUS``: everything libjpeg would only warn about).  stats gains ``jpeg_decoded`` and, per chunk that has JPEG files,
``jpeg_ms``.  Off (the default), nothing changes.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from operator import attrgetter
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from yogo_amd import _hip, png
from yogo_amd.device_decode import MAX_THREADS, png_unpack_any, png_unpack_planes, resize_aa
from yogo_amd.png_batch import KIND_PLANAR, PngStream, _file_size, batch_layout, inflate_batch, jpeg_batch, read_jpeg_stream, read_stream, \
    slot_layout, unpack_table, upload_host_parts
from yogo_amd.resize import aa_taps, device_serves

# images per decode chunk, from tools/bench_prefill.py's sweep (profiles/prefill_decode.log: 772 x 1032 frames, three runs per size):
# every run at 1 024 beat every run at 256 on the noise frames; against 2 048 and 4 096 the prefill times lie inside their scatter
# (the host threads bound it) and the scratch decides: 1.45 GiB device + 1.38 GiB pinned at 1 024, 2.90 + 2.75 GiB at 2 048
DEFAULT_DECODE_BATCH = 1024
MAX_DECODE_BATCH = 65535


def check_decode_batch(decode_batch: int) -> int:
    n = int(decode_batch)
    if not 1 <= n <= MAX_DECODE_BATCH:
        raise ValueError(f"decode_batch {decode_batch} outside [1, {MAX_DECODE_BATCH}]")
    return n


def _label_rows(ds, j: int):
    try:
        return ds.label_rows(j).reshape(-1, 5).to(torch.float32)
    except Exception as e:   # raised when (and only if) the sample becomes resident, as on the host route
        return e


def _host_sample(ds, j: int, rows=None) -> PngStream:
    """the sample through ``ds.image_uint8`` (``pixels`` None: nothing can decode it); ``rows``: its label rows where they are parsed"""
    s = PngStream(host=True, pixels=ds.image_uint8(j))
    s.rows = _label_rows(ds, j) if s.pixels is not None and rows is None else rows
    return s


def _read(ds, j: int, room: np.ndarray, image_hw: Tuple[int, int], decodable: Callable[[png.PngInfo], bool] = attrgetter("prefill_decodable"),
          device_resize: bool = False, jpeg_planes: int = 0) -> PngStream:
    """(pool thread) one sample: its file's zlib stream into ``room`` (its bytes of the pinned slot) and its label rows, or its
    pixels from the host decoder.  decodable: the formats the chunk's unpack kernel takes; device_resize: a file of another size than
    ``image_hw`` stays on the device when the resize kernel serves both of its scales; jpeg_planes: 1 or 3 -- what is no PNG is
    looked at as a JPEG, and one the device decodes gets a record with that many planes (0: it is the host's)"""
    def accept(info, decodable=decodable) -> bool:
        resized = (info.height, info.width) != tuple(image_hw)
        return decodable(info) and (not resized or (device_resize and device_serves(info.height, image_hw[0]) and device_serves(info.width, image_hw[1])))

    # the host decoder's: an unreadable file, another format under its name (png.NotPng), a PNG that does not parse or has no plain
    # zlib wrapper, one the device does not take, one longer than its room (the file grew after its size was taken)
    try:
        with open(str(ds._image_paths[j]), "rb") as f:
            data = f.read()
        try:
            s = read_stream(data, room, accept)
        except png.NotPng:
            if not jpeg_planes:
                raise
            s = read_jpeg_stream(data, room, lambda info: accept(info, attrgetter("device_decodable")), jpeg_planes)
    except (OSError, ValueError):
        return _host_sample(ds, j)
    s.resize = s.hw != tuple(image_hw)
    s.rows = _label_rows(ds, j)
    return s


class Filler:
    """The scratch of ``fill`` kept between calls, for a caller that fills again and again (yogo_amd/image_stream.py: once per decode
    group, every epoch): the two pinned slots, the device buffers of the stored streams and of the scanlines, the two thread pools and
    the side stream.  Nothing is allocated before the first ``fill`` that has samples; the buffers only grow (a slot that has to grow a
    second time takes an eighth more than it needs); ``close()`` gives everything back.  One ``fill`` at a time."""

    def __init__(self, device, max_threads: int = MAX_THREADS):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.threads = max(1, min(MAX_THREADS, int(max_threads), os.cpu_count() or 1))
        self._pool: Optional[ThreadPoolExecutor] = None
        self._stager: Optional[ThreadPoolExecutor] = None
        self._pinned: List[torch.Tensor] = []
        self._sdev: Optional[torch.Tensor] = None
        self._scan: Optional[torch.Tensor] = None
        self._side: Optional[torch.cuda.Stream] = None
        self._staged = 0   # the most bytes a chunk's other-size files took, unpacked, while they waited for their resize

    @property
    def side(self) -> torch.cuda.Stream:
        """the stream every fill runs on"""
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    @property
    def device_bytes(self) -> int:
        return (self._sdev.numel() if self._sdev is not None else 0) + (self._scan.numel() if self._scan is not None else 0) + self._staged

    @property
    def pinned_bytes(self) -> int:
        return sum(t.numel() for t in self._pinned)

    def close(self) -> None:
        """the pools down, the buffers back (after the side stream has finished with them)"""
        for pool in (self._stager, self._pool):
            if pool is not None:
                pool.shutdown(wait=True)
        if self._side is not None:
            self._side.synchronize()
        self._pool = self._stager = self._sdev = self._scan = None
        self._pinned = []

    def _slots(self, slot_bytes: int, count: int) -> None:
        """`count` pinned slots and the device buffer, each of at least `slot_bytes` (side stream current)"""
        have = self._pinned[0].numel() if self._pinned else 0
        if have < slot_bytes:
            count, size = max(count, len(self._pinned)), slot_bytes + (slot_bytes // 8 if have else 0)
            self._pinned, self._sdev = [], None   # (the smaller ones go back first)
            self._pinned = [torch.empty(size, dtype=torch.uint8).pin_memory() for _ in range(count)]
            self._sdev = torch.empty(size, dtype=torch.uint8, device=self.device)
        while len(self._pinned) < count:
            self._pinned.append(torch.empty(self._pinned[0].numel(), dtype=torch.uint8).pin_memory())

    def fill(self, images: torch.Tensor, samples: Sequence[Tuple[object, int]], decode_batch: int = DEFAULT_DECODE_BATCH,
             stats: Optional[Dict] = None, device_resize: bool = False, decode_all: bool = False, raise_rows: bool = True,
             after: Optional[torch.cuda.Event] = None, decode_jpeg: bool = False) -> List[Optional[torch.Tensor]]:
        """the module's ``fill`` on this object's scratch.  raise_rows False: a usable sample whose label file does not parse has its
        exception in the result, in its rows' place, and nothing is raised for it.  after: the side stream waits for this event before
        it touches ``images`` (None: for everything the caller's current stream holds so far)."""
        _hip.require_cuda(images, "the image cache")
        if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[1] not in (1, 3) or not images.is_contiguous():
            raise ValueError(f"fill: images must be a contiguous uint8 [N, 1 or 3, H, W] tensor, got {tuple(images.shape)} {images.dtype}")
        N, C, H, W = (int(v) for v in images.shape)
        if len(samples) != N:
            raise ValueError(f"fill: {len(samples)} samples for {N} images")
        decode_batch = check_decode_batch(decode_batch)
        decodable, unpack = (attrgetter("any_decodable"), png_unpack_any) if decode_all else (attrgetter("prefill_decodable"), png_unpack_planes)
        dev = images.device
        if dev != self.device:
            raise ValueError(f"fill: the images are on {dev}, this filler's scratch on {self.device}")
        out: List[Optional[torch.Tensor]] = [None] * N
        if stats is not None:
            stats.update(scratch_device_bytes=0, scratch_pinned_bytes=0, host_decoded=0, inflate_ms=[], unpack_ms=[], device_resized=0, resize_ms=[])
            if decode_jpeg:
                stats.update(jpeg_decoded=0, jpeg_ms=[])
        if N == 0:
            return out
        chunks = [(lo, min(lo + decode_batch, N)) for lo in range(0, N, decode_batch)]
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="png-prefill")
            self._stager = ThreadPoolExecutor(max_workers=1, thread_name_prefix="png-prefill-stage")   # chunk n + 1 is read while n decodes
        pool, stager = self._pool, self._stager
        sizes = list(pool.map(_file_size, [str(ds._image_paths[j]) for ds, j in samples]))
        layouts = [slot_layout(sizes[lo:hi]) for lo, hi in chunks]
        slot_bytes = max(1, max(total for _, total in layouts))
        side = self.side
        if after is None:
            side.wait_stream(torch.cuda.current_stream(dev))
        else:
            side.wait_event(after)
        images.record_stream(side)
        pending = None
        try:
            with torch.cuda.device(dev), torch.cuda.stream(side):
                self._slots(slot_bytes, min(2, len(chunks)))
                pinned, sdev = self._pinned, self._sdev

                def stage(n: int) -> List[PngStream]:
                    (lo, hi), (offsets, _) = chunks[n], layouts[n]
                    host = pinned[n % 2].numpy()
                    futures = [pool.submit(_read, *samples[i], host[int(offsets[i - lo]):int(offsets[i - lo]) + sizes[i]], (H, W), decodable, device_resize,
                                           C if decode_jpeg else 0)
                               for i in range(lo, hi)]
                    return [f.result() for f in futures]

                pending = stager.submit(stage, 0)
                for n, (lo, hi) in enumerate(chunks):
                    chunk, pending = pending.result(), None
                    if n + 1 < len(chunks):
                        pending = stager.submit(stage, n + 1)
                    self._scan, staging = _decode(chunk, samples[lo:hi], layouts[n], pinned[n % 2], sdev, self._scan, images[lo:hi], stats, unpack)
                    self._staged = max(self._staged, staging)
                    for i, s in enumerate(chunk):
                        if s.host and s.pixels is None:
                            continue
                        if isinstance(s.rows, BaseException) and raise_rows:
                            raise s.rows
                        out[lo + i] = s.rows
                side.synchronize()
        finally:
            if pending is not None:   # (an error left the next chunk being read: the slot is free again only when that has ended)
                pending.exception()
        if stats is not None:
            stats["scratch_device_bytes"] = self.device_bytes
            stats["scratch_pinned_bytes"] = self.pinned_bytes
        return out


def fill(images: torch.Tensor, samples: Sequence[Tuple[object, int]], decode_batch: int = DEFAULT_DECODE_BATCH,
         stats: Optional[Dict] = None, device_resize: bool = False, decode_all: bool = False, decode_jpeg: bool = False) -> List[Optional[torch.Tensor]]:
    """images[i] = the uint8 image of samples[i] = (ObjectDetectionDataset, index in it), what ``ds.image_uint8(index)`` gives, for
    every sample that can be read.  images: contiguous uint8 [N, C, H, W] on an MI355X device (a view of the cache), C 1 or 3.
    -> per sample its fp32 [n, 5] label rows, or None for a sample nothing could decode (its image is left as it was).  Returns after
    the device has finished.  stats (optional dict) receives ``scratch_device_bytes``, ``scratch_pinned_bytes``, ``host_decoded`` and
    per chunk the device-event times ``inflate_ms`` / ``unpack_ms``.  device_resize: files of another size are resized on the device
    (see the module's text); stats then also counts them (``device_resized``) and times every resize launch (``resize_ms``).
    decode_all: every PNG colour type, bit depth and Adam7 is decoded on the device (see the module's text).  decode_jpeg: baseline
    JPEG files are decoded on the device too; stats then also has ``jpeg_decoded`` and ``jpeg_ms``.
    A ``Filler`` that lives for this one call: its scratch is gone when the call returns."""
    _hip.require_cuda(images, "the image cache")
    filler = Filler(images.device)
    try:
        return filler.fill(images, samples, decode_batch, stats, device_resize=device_resize, decode_all=decode_all, decode_jpeg=decode_jpeg)
    finally:
        filler.close()


def _decode(chunk: List[PngStream], samples, layout, pinned: torch.Tensor, sdev: torch.Tensor, scan: Optional[torch.Tensor],
            out: torch.Tensor, stats: Optional[Dict], unpack=png_unpack_planes) -> Tuple[torch.Tensor, int]:
    """one chunk on the current (side) stream: upload, inflate, unpack into ``out`` with the launch wrapper ``unpack`` (the files of
    another size: into a staging tensor per size, resized from there into ``out``), the statuses back; then whatever the device
    refused through the host decoder.  -> the scanline buffer (grown when this chunk needed more), the staging bytes this chunk took"""
    offsets, _ = layout
    B, C, H, W = (int(v) for v in out.shape)
    dev = out.device
    # every image at its own inflated size; behind the last one the palettes of the chunk's palette files, 768 bytes each
    where = batch_layout(chunk, C * H * W)
    if scan is None or scan.numel() < where.total:
        scan = None   # (the smaller buffer goes back to the allocator first)
        scan = torch.empty(where.total, dtype=torch.uint8, device=dev)
    if all(s.host and s.pixels is None for s in chunk):
        return scan, 0
    timed = stats is not None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)] if timed else None
    inflate_status, png_rows = inflate_batch(chunk, offsets, where, pinned, sdev, scan, ev)
    jpeg_status, jpeg_rows = jpeg_batch(chunk, offsets, where, sdev, scan, C, ev[4:] if timed else None)
    device_rows = sorted(png_rows + jpeg_rows)   # the records the device decodes: their stored bytes are in the slot
    for i, s in enumerate(chunk):
        if s.pixels is not None and tuple(s.pixels.shape) != (C, H, W):
            raise ValueError(f"fill: {samples[i][0]._image_paths[samples[i][1]]} decodes to {tuple(s.pixels.shape)}, the cache holds {(C, H, W)}")
    upload_host_parts(chunk, where, scan)
    # a sample nothing could decode keeps its place in the launch as an entry the kernel refuses before it reads anything, and so
    # does a file of another size: its group's own launches follow
    refused = {i for i, s in enumerate(chunk) if s.resize or (s.host and s.pixels is None)}
    table_dev = torch.from_numpy(unpack_table(unpack, chunk, where, refused=refused)).to(dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    if timed:
        ev[2].record()
    unpack(scan, table_dev, (H, W), out, status)
    if timed:
        ev[3].record()
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i in device_rows:
        if chunk[i].resize:
            groups.setdefault(chunk[i].hw, []).append(i)
    resized, staging = [], 0
    for (Hs, Ws), members in groups.items():
        stage = torch.empty((len(members), C, Hs, Ws), dtype=torch.uint8, device=dev)
        staging += stage.numel()
        gstatus = torch.empty(len(members), dtype=torch.int32, device=dev)
        unpack(scan, torch.from_numpy(unpack_table(unpack, chunk, where, rows=members)).to(dev), (Hs, Ws), stage, gstatus)
        gev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timed else None
        if timed:
            gev[0].record()
        # (a file the unpack refused is resized as well, from whatever its staging holds, and overwritten by the host's below)
        resize_aa(stage, out, members, aa_taps(Hs, H), aa_taps(Ws, W))
        if timed:
            gev[1].record()
        resized.append((members, gstatus, gev))
    bad = status.cpu().numpy().copy()   # waits for the launches
    for members, gstatus, gev in resized:
        bad[members] = gstatus.cpu().numpy()
        if timed:
            stats["resize_ms"].append(gev[0].elapsed_time(gev[1]))
    if inflate_status is not None:
        bad[np.asarray(png_rows)[inflate_status.cpu().numpy() != 0]] = 1
    if jpeg_status is not None:
        bad[np.asarray(jpeg_rows)[jpeg_status.cpu().numpy() != 0]] = 1
    if timed:
        if png_rows:
            stats["inflate_ms"].append(ev[0].elapsed_time(ev[1]))
        if jpeg_rows:
            stats["jpeg_ms"].append(ev[4].elapsed_time(ev[5]))
            stats["jpeg_decoded"] += sum(1 for i in jpeg_rows if not bad[i])
        stats["unpack_ms"].append(ev[2].elapsed_time(ev[3]))
        stats["host_decoded"] += sum(1 for s in chunk if s.host)
        stats["device_resized"] += sum(1 for i in device_rows if chunk[i].resize and not bad[i])
    # what the device refused: the host decoder's turn (the kernel may have written part of the image: it is overwritten or,
    # where the host cannot read the file either, not resident)
    for i in device_rows:
        if not bad[i]:
            continue
        s = chunk[i] = _host_sample(*samples[i], rows=chunk[i].rows)
        if timed:
            stats["host_decoded"] += 1
        if s.pixels is None:
            continue
        px = s.pixels.contiguous().reshape(-1).to(dev)
        one = torch.tensor([[0, KIND_PLANAR]], dtype=torch.int64).to(dev)
        st = torch.empty(1, dtype=torch.int32, device=dev)
        png_unpack_planes(px, one, (H, W), out[i:i + 1], st)
        if int(st.cpu()[0]) != 0:
            raise RuntimeError(f"yogo_amd: the host-decoded image of {samples[i][0]._image_paths[samples[i][1]]} was refused by the unpack kernel")
    return scan, staging
