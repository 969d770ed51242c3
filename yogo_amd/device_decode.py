"""What the routes that decode stored bytes on the device share -- zarr stacks (yogo_amd/zarr_feed.py), PNG directories for inference
(yogo_amd/png_feed.py) and the PNG prefill of the device image cache (yogo_amd/png_prefill.py), both on yogo_amd/png_batch.py: the launch wrappers of
``yogo_blosc_lz4_decode``, ``yogo_zstd_decode``, ``yogo_inflate_zlib``, ``yogo_png_unpack``, ``yogo_png_unpack_planes``, ``yogo_png_unpack_any`` and ``yogo_resize_aa_u8`` (the
prefill's resize of other-size files) with their tensor checks, ``gather`` (a pool's futures), ``raise_first_bad`` (a status vector -> RuntimeError), ``png_stream_into`` (one PNG file -> one zlib
stream in its room of a pinned slot), ``feed_device`` (the checks of the feeds' constructors) and ``PrefetchFeed`` (the iterator that
loads batch n + 1 while the caller works on batch n)."""
from __future__ import annotations

from concurrent.futures import Future, ThreadPoolExecutor
from typing import Callable, Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from yogo_amd import _hip, inflate

ALIGN = 256          # every staged chunk / stored stream starts on a multiple of this (the kernels ask for 16)
MAX_THREADS = 16


def center_crop_origin(H: int, W: int, OH: int, OW: int) -> Tuple[int, int]:
    """(top, left) of torchvision's CenterCrop((OH, OW)) on an H x W image (yogo_amd.image_path_dataset.CenterCrop)"""
    if OH > H or OW > W or OH < 1 or OW < 1:
        raise ValueError(f"crop {(OH, OW)} does not fit the image {(H, W)}")
    return int(round((H - OH) / 2.0)), int(round((W - OW) / 2.0))


def feed_device(device, batch_size: int, what: str) -> torch.device:
    """(the feeds' constructors) ``device`` as a torch.device with its index; RuntimeError where it is no MI355X device (``what``: "the
    zarr feed unpacks"), ValueError for a batch size a launch's grid does not take"""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"yogo_amd: {what} on an MI355X device (got {dev}); there is no CPU fallback")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if batch_size < 1 or batch_size > 65535:
        raise ValueError(f"batch size {batch_size} outside [1, 65535]")
    return dev


def require_bytes(who: str, what: str, *tensors: torch.Tensor) -> None:
    """(the launch wrappers' tensor checks: ``who`` is the wrapper's name in the message)  every tensor a non-empty contiguous 1-D uint8
    one; ``what`` names it (them)"""
    for t in tensors:
        if t.dtype != torch.uint8 or t.ndim != 1 or not t.is_contiguous() or t.numel() == 0:
            if len(tensors) > 1:
                raise ValueError(f"{who}: {what} must be non-empty contiguous 1-D uint8 tensors")
            raise ValueError(f"{who}: {what} must be a non-empty contiguous 1-D uint8 tensor, got {tuple(t.shape)} {t.dtype}")


def require_table(who: str, table: torch.Tensor, k: int, n: Optional[int] = None) -> None:
    """a contiguous int64 [n, k] table; n None: any number of rows"""
    if table.dtype != torch.int64 or table.ndim != 2 or table.shape[1] != k or n not in (None, table.shape[0]) or not table.is_contiguous():
        raise ValueError(f"{who}: the table must be a contiguous int64 [{'n' if n is None else n}, {k}] tensor, got {tuple(table.shape)} {table.dtype}")


def require_status(who: str, status: torch.Tensor, n: int) -> None:
    if status.dtype != torch.int32 or tuple(status.shape) != (n,) or not status.is_contiguous():
        raise ValueError(f"{who}: the status must be a contiguous int32 [{n}] tensor, got {tuple(status.shape)} {status.dtype}")


def require_same_device(who: str, *tensors: torch.Tensor) -> None:
    if len({t.device for t in tensors}) != 1:
        raise ValueError(f"{who}: the tensors live on different devices")


def _decode_rows(symbol: str, stored: torch.Tensor, table: torch.Tensor, out: torch.Tensor, status: torch.Tensor,
                 work: Optional[torch.Tensor] = None) -> None:
    """one launch of a device decoder (`symbol`): the checks they share.  work: the workspace of a decoder that takes one"""
    what = symbol[len("yogo_"):]
    extra = () if work is None else (work,)
    for t, name in ((stored, "the stored chunk bytes"), (table, "the table"), (out, "the decoded chunks"), (status, "the status"),
                    (work, "the workspace"))[:4 + len(extra)]:
        _hip.require_cuda(t, name)
    require_bytes(what, "stored and out" if work is None else "stored, out and work", stored, out, *extra)
    n = int(table.shape[0])
    require_table(what, table, 5)
    require_status(what, status, n)
    require_same_device(what, stored, table, out, status, *extra)
    if n == 0:
        return
    if work is not None and work.numel() < zstd_work_bytes(n):
        raise ValueError(f"{what}: a workspace of {work.numel()} bytes for {n} rows, {zstd_work_bytes(n)} needed")
    with torch.cuda.device(out.device):
        if work is None:
            _hip.call(symbol, stored, stored.numel(), table, n, out, out.numel(), status, _hip.stream_ptr())
        else:
            _hip.call(symbol, stored, stored.numel(), table, n, out, out.numel(), status, work, work.numel(), _hip.stream_ptr())


def decode_blocks(stored: torch.Tensor, table: torch.Tensor, out: torch.Tensor, status: torch.Tensor) -> None:
    """One ``yogo_blosc_lz4_decode`` launch on the current stream.  stored / out: 1-D uint8 device tensors (stored chunk bytes, decoded
    staging buffer); table: int64 [n, 5] device, rows (src_off, src_len, dst_off, dst_len, raw); status: int32 [n] device.  The
    kernel holds every row to the two buffers itself."""
    _decode_rows("yogo_blosc_lz4_decode", stored, table, out, status)


def inflate_streams(stored: torch.Tensor, table: torch.Tensor, out: torch.Tensor, status: torch.Tensor) -> None:
    """One ``yogo_inflate_zlib`` launch on the current stream; as decode_blocks, rows (src_off, src_len, dst_off, dst_len, adler32):
    the raw DEFLATE bytes of one zlib stream each (yogo_amd.inflate.split_zlib)."""
    _decode_rows("yogo_inflate_zlib", stored, table, out, status)


def zstd_work_bytes(n: int) -> int:
    """the workspace ``zstd_frames`` needs for a table of n rows (``yogo_zstd_work_bytes``: 128 KB per row)"""
    return _hip.query_size("yogo_zstd_work_bytes", int(n))


def zstd_frames(stored: torch.Tensor, table: torch.Tensor, out: torch.Tensor, status: torch.Tensor, work: torch.Tensor) -> None:
    """One ``yogo_zstd_decode`` launch on the current stream; as decode_blocks, rows (src_off, src_len, dst_off, dst_len, raw): one
    Zstandard frame each (a Blosc-zstd block, a chunk of the ``zstd`` codec), or raw bytes.  work: a 1-D uint8 device tensor of at
    least ``zstd_work_bytes(n)`` bytes (a block's Huffman-coded literals, per row)."""
    _decode_rows("yogo_zstd_decode", stored, table, out, status, work)


JPEG_TABLE_COLS = 18   # yogo_amd.jpeg.TABLE_COLS


def jpeg_decode(stored: torch.Tensor, table: torch.Tensor, out: torch.Tensor, planes: int, status: torch.Tensor) -> None:
    """One ``yogo_jpeg_decode`` launch on the current stream.  stored: 1-D uint8 device tensor, the files as they came off the disk;
    table: int64 [n, 18] device, rows of ``yogo_amd.jpeg.table_row``; out: 1-D uint8 device tensor, where every file's
    [planes][H][W] bytes go (planes 1 or 3); status: int32 [n] device.  The kernel holds every row to the two buffers itself."""
    for t, name in ((stored, "the stored files"), (table, "the table"), (out, "the decoded planes"), (status, "the status")):
        _hip.require_cuda(t, name)
    require_bytes("jpeg_decode", "stored and out", stored, out)
    if planes not in (1, 3):
        raise ValueError(f"jpeg_decode: {planes} planes, 1 or 3 are written")
    n = int(table.shape[0])
    require_table("jpeg_decode", table, JPEG_TABLE_COLS)
    require_status("jpeg_decode", status, n)
    require_same_device("jpeg_decode", stored, table, out, status)
    if n == 0:
        return
    with torch.cuda.device(out.device):
        _hip.call("yogo_jpeg_decode", stored, stored.numel(), table, n, out, out.numel(), int(planes), status, _hip.stream_ptr())


def png_unpack(scan: torch.Tensor, table: torch.Tensor, image_hw: Tuple[int, int], out: torch.Tensor, status: torch.Tensor,
               top: int = 0, left: int = 0) -> torch.Tensor:
    """One ``yogo_png_unpack`` launch on the current stream.  scan: 1-D uint8 device tensor of inflated scanlines (written: the
    kernel unfilters one row of every 64 in place); table: int64 [B, 2] device, rows (offset, raw); out: contiguous [B, 1, OH, OW]
    uint8 or float32; status: int32 [B].  The kernel holds every image to ``scan`` itself."""
    for t, what in ((scan, "the scanlines"), (table, "the image table"), (out, "the unpack output"), (status, "the status")):
        _hip.require_cuda(t, what)
    H, W = (int(v) for v in image_hw)
    require_bytes("png_unpack", "scan", scan)
    if out.dtype not in (torch.uint8, torch.float32) or out.ndim != 4 or out.shape[1] != 1 or not out.is_contiguous():
        raise ValueError(f"png_unpack: out must be a contiguous [B, 1, OH, OW] uint8 or float32 tensor, got {tuple(out.shape)} {out.dtype}")
    B, _, OH, OW = (int(v) for v in out.shape)
    require_table("png_unpack", table, 2, B)
    require_status("png_unpack", status, B)
    require_same_device("png_unpack", scan, table, out, status)
    if B == 0:
        return out
    with torch.cuda.device(out.device):
        _hip.call("yogo_png_unpack", scan, scan.numel(), table, B, H, W, int(top), int(left), OH, OW, out,
                  1 if out.dtype == torch.float32 else 0, status, _hip.stream_ptr())
    return out


def png_unpack_planes(scan: torch.Tensor, table: torch.Tensor, image_hw: Tuple[int, int], out: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
    """One ``yogo_png_unpack_planes`` launch on the current stream.  scan: 1-D uint8 device tensor (written: the kernel unfilters one
    row of every 64 in place); table: int64 [B, 2] device, rows (offset, kind); out: contiguous uint8 [B, C, H, W], C 1 or 3;
    status: int32 [B].  The kernel holds every image to ``scan`` itself."""
    for t, what in ((scan, "the scanlines"), (table, "the image table"), (out, "the unpack output"), (status, "the status")):
        _hip.require_cuda(t, what)
    H, W = (int(v) for v in image_hw)
    require_bytes("png_unpack_planes", "scan", scan)
    if out.dtype != torch.uint8 or out.ndim != 4 or out.shape[1] not in (1, 3) or tuple(out.shape[2:]) != (H, W) or not out.is_contiguous():
        raise ValueError(f"png_unpack_planes: out must be a contiguous uint8 [B, 1 or 3, {H}, {W}] tensor, got {tuple(out.shape)} {out.dtype}")
    B, C = int(out.shape[0]), int(out.shape[1])
    require_table("png_unpack_planes", table, 2, B)
    require_status("png_unpack_planes", status, B)
    require_same_device("png_unpack_planes", scan, table, out, status)
    if B == 0:
        return out
    with torch.cuda.device(out.device):
        _hip.call("yogo_png_unpack_planes", scan, scan.numel(), table, B, H, W, C, out, status, _hip.stream_ptr())
    return out


def png_unpack_any(scan: torch.Tensor, table: torch.Tensor, image_hw: Tuple[int, int], out: torch.Tensor, status: torch.Tensor,
                   top: int = 0, left: int = 0) -> torch.Tensor:
    """One ``yogo_png_unpack_any`` launch on the current stream: PNG scanlines of every colour type, bit depth and interlace method.
    scan: 1-D uint8 device tensor of inflated scanlines and palettes (written: the kernel unfilters one row of every 64 in place);
    table: int64 [B, 3] device, rows (offset, ``PngInfo.format_code`` or ``png.FMT_PLANAR``, offset of the 768-byte palette);
    out: contiguous [B, 1 or 3, OH, OW] uint8 or float32, the crop at (top, left) of the H x W images; status: int32 [B].  The
    kernel holds every image and palette to ``scan`` itself."""
    for t, what in ((scan, "the scanlines"), (table, "the image table"), (out, "the unpack output"), (status, "the status")):
        _hip.require_cuda(t, what)
    H, W = (int(v) for v in image_hw)
    require_bytes("png_unpack_any", "scan", scan)
    if out.dtype not in (torch.uint8, torch.float32) or out.ndim != 4 or out.shape[1] not in (1, 3) or not out.is_contiguous():
        raise ValueError(f"png_unpack_any: out must be a contiguous [B, 1 or 3, OH, OW] uint8 or float32 tensor, got {tuple(out.shape)} {out.dtype}")
    B, C, OH, OW = (int(v) for v in out.shape)
    require_table("png_unpack_any", table, 3, B)
    require_status("png_unpack_any", status, B)
    require_same_device("png_unpack_any", scan, table, out, status)
    if B == 0:
        return out
    with torch.cuda.device(out.device):
        _hip.call("yogo_png_unpack_any", scan, scan.numel(), table, B, H, W, int(top), int(left), OH, OW, C, out,
                  1 if out.dtype == torch.float32 else 0, status, _hip.stream_ptr())
    return out


def resize_aa(src: torch.Tensor, dst: torch.Tensor, dst_index, taps_y: Tuple[np.ndarray, np.ndarray],
              taps_x: Tuple[np.ndarray, np.ndarray]) -> torch.Tensor:
    """One ``yogo_resize_aa_u8`` launch on the current stream: dst[dst_index[k]] = src[k] resampled as ``resize_image`` does it.
    src: contiguous uint8 [n, C, Hs, Ws] device; dst: contiguous uint8 [N, C, Hd, Wd] on the same device; dst_index: n distinct
    slots of dst (a sequence or an int64 tensor, on the host); taps_y / taps_x: ``yogo_amd.resize.aa_taps(Hs, Hd)`` / ``(Ws, Wd)``,
    (start int32 [n_out], weights float32 [n_out, K]).  The entry point checks the tables and the slots before it launches."""
    for t, what in ((src, "the source images"), (dst, "the resized images")):
        _hip.require_cuda(t, what)
    for t, name in ((src, "src"), (dst, "dst")):
        if t.dtype != torch.uint8 or t.ndim != 4 or not t.is_contiguous() or t.numel() == 0:
            raise ValueError(f"resize_aa: {name} must be a non-empty contiguous uint8 [n, C, H, W] tensor, got {tuple(t.shape)} {t.dtype}")
    if src.shape[1] != dst.shape[1]:
        raise ValueError(f"resize_aa: src has {src.shape[1]} planes, dst {dst.shape[1]}")
    require_same_device("resize_aa", src, dst)
    n, C, Hs, Ws = (int(v) for v in src.shape)
    N, _, Hd, Wd = (int(v) for v in dst.shape)
    index = np.ascontiguousarray(torch.as_tensor(dst_index, dtype=torch.int64).reshape(-1).cpu().numpy())
    if index.size != n:
        raise ValueError(f"resize_aa: {index.size} destination slots for {n} images")
    parts = [index]
    for (start, weights), n_out, axis in ((taps_y, Hd, "y"), (taps_x, Wd, "x")):
        start, weights = np.asarray(start), np.asarray(weights)
        if start.dtype != np.int32 or start.shape != (n_out,) or weights.dtype != np.float32 or weights.ndim != 2 or weights.shape[0] != n_out \
                or weights.shape[1] < 1:
            raise ValueError(f"resize_aa: the {axis} taps must be (int32 [{n_out}], float32 [{n_out}, K]), got {start.dtype} {start.shape}, "
                             f"{weights.dtype} {weights.shape}")
    (sy, wy), (sx, wx) = taps_y, taps_x
    parts += [np.ascontiguousarray(sy), np.ascontiguousarray(sx), np.ascontiguousarray(wy), np.ascontiguousarray(wx)]
    packed = np.concatenate([p.reshape(-1).view(np.uint8) for p in parts])
    host = np.zeros(-(-packed.size // 8), dtype=np.int64)   # (8-byte aligned, as the entry point asks)
    host.view(np.uint8)[:packed.size] = packed
    with torch.cuda.device(dst.device):
        _hip.call("yogo_resize_aa_u8", src, n, C, Hs, Ws, dst, N, Hd, Wd, host.ctypes.data, torch.from_numpy(host).to(dst.device),
                  int(np.asarray(wy).shape[1]), int(np.asarray(wx).shape[1]), _hip.stream_ptr())
    return dst


def gather(futures: Sequence[Future]) -> list:
    """every future's result, in order -- or, after every future has ended, the first one's exception"""
    for e in [f.exception() for f in futures]:   # (the list: every future has ended before the first error is raised)
        if e is not None:
            raise e
    return [f.result() for f in futures]


def raise_first_bad(status: Optional[torch.Tensor], texts: Mapping[int, str], name_of_row: Callable[[int], str]) -> None:
    """status: what a decode launch left per row, on the host (None: there was no launch).  The first non-zero entry becomes the
    RuntimeError naming its row (``name_of_row(i)``: a file, a chunk of a store) and the status' words from ``texts``"""
    if status is None or not bool(status.any()):
        return
    first = int(torch.nonzero(status)[0])
    code = int(status[first])
    raise RuntimeError(f"{name_of_row(first)} could not be decoded on the device ({texts.get(code, 'unknown status')}: status {code})")


def png_stream_into(data: bytes, info, room: np.ndarray) -> Tuple[int, int, int, int]:
    """The IDAT payloads of one parsed PNG file (``info = png.parse_png(data)``) back to back at the start of ``room`` -- one zlib stream
    -- and the wrapper taken off: -> (stored bytes, where the raw DEFLATE bytes start in them, how many, the Adler-32).  The caller has
    made sure that ``info.idat_bytes`` fit; ValueError (yogo_amd.inflate.split_zlib) for a wrapper that is no plain zlib one."""
    at = 0
    for o, n in info.idat:
        room[at:at + n] = np.frombuffer(data, dtype=np.uint8, count=n, offset=o)
        at += n
    off, ln, adler = inflate.split_zlib(room[:at])
    return at, off, ln, adler


class PrefetchFeed:
    """Iterator over ``self.batches`` ([lo, hi) of ``count`` items, ``batch_size`` at a time) that has batch n + 1 loading while the
    caller works on batch n.  A subclass gives ``_load(n)`` (on the one loader thread: loads run one after the other) and
    ``_deliver(n, loaded)`` (on the caller's thread: what ``next()`` returns).  An object, not a generator: when a batch raises
    RuntimeError, the next ``next()`` goes on with the following batch.  ``close()`` runs when the batches are used up."""

    def __init__(self, count: int, batch_size: int, thread_name: str):
        self.batches = [(lo, min(lo + batch_size, count)) for lo in range(0, count, batch_size)]
        self._loader = ThreadPoolExecutor(max_workers=1, thread_name_prefix=thread_name)
        self._pending: Dict[int, Future] = {}
        self._pos = 0

    def __len__(self) -> int:
        return len(self.batches)

    def __iter__(self):
        return self

    def close(self) -> None:
        for f in self._pending.values():
            f.cancel()
        self._loader.shutdown(wait=True)
        self._pending.clear()

    def __next__(self):
        if self._pos >= len(self.batches):
            self.close()
            raise StopIteration
        n = self._pos
        self._pos += 1
        fut = self._pending.pop(n, None) or self._loader.submit(self._load, n)
        if n + 1 < len(self.batches):
            self._pending[n + 1] = self._loader.submit(self._load, n + 1)
        return self._deliver(n, fut.result())
