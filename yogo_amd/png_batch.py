"""One batch of PNG files decoded on the device: what the inference feed (yogo_amd/png_feed.py) and the prefill of the device image
cache (yogo_amd/png_prefill.py) both do between a file's bytes and the unpack launch.

  ``read_stream``     file bytes + the file's room in a pinned slot -> a ``PngStream``: the IDAT payloads back to back in the room
                      (one zlib stream, ``device_decode.png_stream_into``), where the DEFLATE bytes lie, what they inflate to, the
                      format and the palette.  What the caller's predicate does not accept raises ``Refused``.
  ``slot_layout``     file sizes -> every file's room in a pinned slot, at multiples of ``ALIGN``
  ``scan_layout``     inflated sizes -> every image's place in the scanline buffer at multiples of ``SCAN_ALIGN``, the palettes of
                      the batch's palette files (768 bytes each) behind the last image
  ``read_jpeg_stream``  the same for a baseline JPEG file (``--device-image-decode-jpeg``): the file's bytes as they are in the room
  ``inflate_batch``   the slot up, ONE ``yogo_inflate_zlib`` launch over the batch's streams (rows of ``inflate_rows``)
  ``jpeg_batch``      ONE ``yogo_jpeg_decode`` launch over the batch's JPEG files: their planes where host pixels would lie
  ``upload_host_parts``  the pixels of the images the host decoded and the palettes into the scanline buffer
  ``unpack_table``    the table of ``yogo_png_unpack`` / ``yogo_png_unpack_planes`` ([B, 2]) or ``yogo_png_unpack_any`` ([B, 3])

What a failure means -- RuntimeError for the feed, the host decoder for the prefill --, which files are accepted and how the slots
are sized stay with the callers."""
from __future__ import annotations

import os
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from yogo_amd import inflate, jpeg, png
from yogo_amd.device_decode import ALIGN, inflate_streams, jpeg_decode, png_stream_into, png_unpack, png_unpack_any, png_unpack_planes

SCAN_ALIGN = 16   # yogo_inflate_zlib asks for 16-byte aligned destinations
KIND_GREY, KIND_PLANAR, KIND_RGB = 0, 1, 2   # yogo_png_unpack_planes' kinds
REFUSED = -1      # a table entry every unpack kernel refuses before it reads anything


class Refused(ValueError):
    """the file is a PNG, but not one the caller's predicate accepts, or its stream is longer than its room: the host's to decode"""


class PngStream:
    """what one file of a batch turned out to be.  For the device: the file's ``hw``, ``stored`` bytes of zlib stream at the start
    of its room, the ``deflate`` range (offset, length) and ``adler`` inside them, ``need`` bytes the stream inflates to, the format
    ``code`` of yogo_png_unpack_any's table, the ``palette`` (768 bytes) of a palette file; ``stream``: the bytes themselves where
    there was no room to copy them to.  For the host (``host``): ``pixels``, what the host decoder gave, None where it gave up.
    The prefill's own: ``rows`` (the sample's label rows, or the exception their parsing raised) and ``resize`` (the file has
    another size than the cache and the device resizes it).  ``jpeg``: the ``JpegInfo`` of a JPEG file the device decodes -- its
    ``stored`` bytes are the whole file, ``need`` its planes * H * W, and the unpack launch sees it as planar pixels (``planar``)."""
    __slots__ = ("hw", "stored", "deflate", "adler", "need", "code", "palette", "stream", "host", "pixels", "rows", "resize", "jpeg")

    def __init__(self, hw=None, stored=0, deflate=(0, 0), adler=0, need=0, code=png.FMT_PLANAR, palette=None, stream=None,
                 host=False, pixels=None, jpeg=None):
        self.hw, self.stored, self.deflate, self.adler, self.need, self.code = hw, stored, deflate, adler, need, code
        self.palette, self.stream, self.host, self.pixels, self.rows, self.resize = palette, stream, host, pixels, None, False
        self.jpeg = jpeg

    @property
    def bpp(self) -> int:
        """bytes per pixel of an 8-bit file (``PngInfo.bytes_per_pixel``): 3 for colour type 2, the low byte of the format code"""
        return 3 if self.code & 0xFF == 2 else 1

    @property
    def planar(self) -> bool:
        """the unpack launch finds [planes][H][W] pixels at the image's place: the host decoded it, or yogo_jpeg_decode did"""
        return self.host or self.jpeg is not None


def _file_size(path: str) -> int:
    try:
        return os.stat(path).st_size
    except OSError:
        return 0


def slot_layout(sizes: Sequence[int]) -> Tuple[np.ndarray, int]:
    """file sizes -> (where each file's room starts in a slot, the bytes the chunk takes): room i holds ``sizes[i]`` bytes and
    starts on a multiple of ALIGN, the rooms in order and without overlap"""
    rooms = (np.asarray(sizes, dtype=np.int64).reshape(-1) + (ALIGN - 1)) // ALIGN * ALIGN
    offsets = np.zeros(len(rooms), dtype=np.int64)
    if len(rooms) > 1:
        offsets[1:] = np.cumsum(rooms[:-1])
    return offsets, int(rooms.sum())


def read_stream(data: bytes, room: Optional[np.ndarray], accept: Callable[[png.PngInfo], bool]) -> PngStream:
    """(pool thread) the bytes of one file -> its record, the zlib stream copied into ``room`` (this file's bytes of a pinned slot;
    None: there is no slot yet and the record keeps the stream as bytes).  ``accept``: which parsed files the caller's unpack kernel
    takes (``PngInfo.device_decodable``, ``.prefill_decodable``, ``.any_decodable``, and whatever else the caller asks of a file).
    Raises png.NotPng (another format under the name), Refused (not accepted, or longer than its room: nothing is copied) and
    ValueError (a PNG that does not parse, a zlib wrapper that is no plain one)."""
    info = png.parse_png(data)
    if not accept(info) or (room is not None and info.idat_bytes > len(room)):
        raise Refused(f"PNG: colour type {info.color_type} at {info.bit_depth} bits, {info.idat_bytes} bytes of IDAT")
    if room is None:
        stream = b"".join(data[o:o + n] for o, n in info.idat)
        stored, (off, ln, adler) = len(stream), inflate.split_zlib(stream)
    else:
        stream = None
        stored, off, ln, adler = png_stream_into(data, info, room)
    return PngStream((info.height, info.width), stored, (off, ln), adler, info.inflated_bytes, info.format_code,
                     png.palette_table(data, info) if info.color_type == 3 else None, stream)


def read_jpeg_stream(data: bytes, room: Optional[np.ndarray], accept: Callable[[jpeg.JpegInfo], bool], planes: int) -> PngStream:
    """(pool thread) ``read_stream`` for a JPEG file: its record, the file's bytes copied into ``room`` as they are (None: the record
    keeps them).  ``accept``: ``JpegInfo.device_decodable`` and whatever else the caller asks of a file; ``planes``: 1 or 3, what the
    batch is converted to.  Raises jpeg.NotJpeg, Refused (not accepted, or longer than its room) and ValueError (does not parse)."""
    info = jpeg.parse_jpeg(data)
    if not accept(info) or (room is not None and len(data) > len(room)):
        raise Refused(f"JPEG: SOF{info.sof}, {len(info.components)} components at {info.precision} bits, {len(data)} bytes")
    if room is not None:
        room[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    return PngStream((info.height, info.width), len(data), need=planes * info.height * info.width, stream=None if room is not None else data,
                     jpeg=info)


class ScanLayout(NamedTuple):
    at: np.ndarray               # int64 [B + 1]: where image i starts in the scanline buffer; at[B]: where the palettes start
    palette_at: Dict[int, int]   # image -> where its palette starts
    total: int                   # bytes of the scanline buffer in use
    need: List[int]              # bytes image i takes: what its stream inflates to, or its host-decoded pixels


def scan_layout(need: Sequence[int], with_palette: Sequence[int] = ()) -> ScanLayout:
    """the bytes every image of a batch takes, and which images bring a palette -> their places: every image on a multiple of
    SCAN_ALIGN, in order and without overlap; directly behind the last image the palettes, PALETTE_BYTES each"""
    at = np.zeros(len(need) + 1, dtype=np.int64)
    at[1:] = np.cumsum([-(-int(v) // SCAN_ALIGN) * SCAN_ALIGN for v in need])
    palette_at = {i: int(at[-1]) + k * png.PALETTE_BYTES for k, i in enumerate(with_palette)}
    return ScanLayout(at, palette_at, int(at[-1]) + len(palette_at) * png.PALETTE_BYTES, [int(v) for v in need])


def batch_layout(records: Sequence[PngStream], host_bytes: int) -> ScanLayout:
    """``scan_layout`` of a batch: a stream at what it inflates to, an image of the host's at ``host_bytes`` (planes * H * W)"""
    return scan_layout([host_bytes if r.host else r.need for r in records], [i for i, r in enumerate(records) if r.palette is not None])


def inflate_rows(records: Sequence[PngStream], src_at: Sequence[int], layout: ScanLayout) -> np.ndarray:
    """``inflate_streams``' table, int64 [n, 5], one row per record that is the device's: (where the DEFLATE bytes start in the slot
    -- ``src_at[i]``: where room i does --, how many, where the scanlines go, how many, the Adler-32)"""
    return np.asarray([(int(src_at[i]) + r.deflate[0], r.deflate[1], int(layout.at[i]), layout.need[i], r.adler)
                       for i, r in enumerate(records) if not r.planar], dtype=np.int64).reshape(-1, 5)


def inflate_batch(records: Sequence[PngStream], src_at: Sequence[int], layout: ScanLayout, pinned: torch.Tensor, sdev: torch.Tensor,
                  scan: torch.Tensor, events=None) -> Tuple[Optional[torch.Tensor], List[int]]:
    """(current stream) the slot's bytes in use up (``pinned`` -> ``sdev``) and ONE yogo_inflate_zlib launch into ``scan``
    -> (its status, int32 per row, None where no record is the device's; which records its rows are).  ``events``: two events
    recorded before and behind the launch.  The JPEG files of the batch go up with the slot and are ``jpeg_batch``'s."""
    device_rows = [i for i, r in enumerate(records) if not r.planar]
    stored = [i for i, r in enumerate(records) if not r.host]
    if not stored:
        return None, device_rows
    used = int(src_at[stored[-1]]) + records[stored[-1]].stored
    sdev[:used].copy_(pinned[:used], non_blocking=True)
    if not device_rows:
        return None, device_rows
    status = torch.empty(len(device_rows), dtype=torch.int32, device=scan.device)
    if events:
        events[0].record()
    inflate_streams(sdev, torch.from_numpy(inflate_rows(records, src_at, layout)).to(scan.device), scan, status)
    if events:
        events[1].record()
    return status, device_rows


def jpeg_batch(records: Sequence[PngStream], src_at: Sequence[int], layout: ScanLayout, sdev: torch.Tensor, scan: torch.Tensor,
               planes: int, events=None) -> Tuple[Optional[torch.Tensor], List[int]]:
    """(current stream, behind ``inflate_batch``, which took the slot up) ONE yogo_jpeg_decode launch over the batch's JPEG files:
    each one's [planes][H][W] bytes into ``scan`` at its place -> (its status, int32 per row, None where the batch has no JPEG
    file; which records its rows are).  ``events``: two events recorded before and behind the launch."""
    rows = [i for i, r in enumerate(records) if r.jpeg is not None]
    if not rows:
        return None, rows
    table = np.asarray([jpeg.table_row(records[i].jpeg, int(src_at[i]), records[i].stored, int(layout.at[i]), planes) for i in rows],
                       dtype=np.int64).reshape(-1, jpeg.TABLE_COLS)
    status = torch.empty(len(rows), dtype=torch.int32, device=scan.device)
    if events:
        events[0].record()
    jpeg_decode(sdev, torch.from_numpy(table).to(scan.device), scan, planes, status)
    if events:
        events[1].record()
    return status, rows


def upload_host_parts(records: Sequence[PngStream], layout: ScanLayout, scan: torch.Tensor) -> None:
    """(current stream) what the host contributes to the scanline buffer: the pixels of the images it decoded (rare: a pageable copy
    per image) and, in one copy, the palettes of the batch"""
    for i, r in enumerate(records):
        if r.pixels is not None:
            scan[int(layout.at[i]):int(layout.at[i]) + layout.need[i]].copy_(torch.as_tensor(r.pixels).contiguous().reshape(-1))
    if layout.palette_at:
        scan[int(layout.at[-1]):layout.total].copy_(torch.from_numpy(np.concatenate([records[i].palette for i in layout.palette_at])))


def unpack_table(kernel, records: Sequence[PngStream], layout: ScanLayout, rows: Optional[Sequence[int]] = None,
                 refused: Sequence[int] = ()) -> np.ndarray:
    """the table of one unpack launch (``kernel``: the launch wrapper) over ``rows`` of the batch (default: all of them), int64:
    (offset, raw) for png_unpack, (offset, kind) for png_unpack_planes, (offset, format code, offset of the palette) for
    png_unpack_any.  ``refused``: records that keep their place in the launch as an entry the kernel refuses."""
    def code(r: PngStream) -> int:
        if kernel is png_unpack:
            return 1 if r.planar else 0
        if kernel is png_unpack_planes:
            return KIND_PLANAR if r.planar else KIND_RGB if r.bpp == 3 else KIND_GREY
        return png.FMT_PLANAR if r.planar else r.code

    width = 3 if kernel is png_unpack_any else 2
    table = [(int(layout.at[i]), REFUSED if i in refused else code(records[i]), layout.palette_at.get(i, 0))[:width]
             for i in (range(len(records)) if rows is None else rows)]
    return np.asarray(table, dtype=np.int64).reshape(-1, width)
