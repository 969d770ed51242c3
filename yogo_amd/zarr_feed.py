"""Inference batches from a zarr stack, unpacked on the device (``yogo infer --path-to-zarr``).

The reference indexes its ZarrDataset per image in the main process (workers forced to 0, yogo/infer.py:257-265) and stacks the
frames on the host.  Here a ``ZarrDeviceFeed`` takes the DataLoader's place: per batch it works out which chunks the frames
``[lo, hi)`` live in, reads and decodes them on a thread pool straight into a pinned staging buffer (an uncompressed chunk with one
copy), uploads the buffer on a side stream and launches ``yogo_zarr_unpack`` (yogo_amd/csrc/zarr_feed.hip) on the compute stream
behind an event: de-interleave / crop / optional ``/ 255`` happen there.  Two staging and two device buffers: the reading and the
upload of batch n+1 overlap whatever the caller does with batch n.  A chunk that two consecutive batches share (more than one
frame per chunk, batch size no multiple of it) is read and decoded once and copied from the previous staging buffer.

Blosc-compressed stacks with LZ4 blocks (zarr's default compressor) are decoded on the device (``device_decode=True``, the
default): the stager reads the STORED bytes into a second pair of pinned buffers and parses each chunk's header into one table
entry per block (yogo_amd/blosc.py), the loader uploads bytes and table, launches ``yogo_blosc_lz4_decode``
(yogo_amd/csrc/blosc_lz4.hip) on the side stream into the slot's device buffer -- the layout ``yogo_zarr_unpack`` reads -- and
waits for the per-block status.  A chunk the device cannot decode (zlib inside, bit-shuffle) is decoded on the host and enters
the table as one raw entry.

Stacks under zarr's ``zlib`` codec take the same route with another decoder: one table row per chunk -- the raw DEFLATE bytes
between the zlib header and trailer, and the trailer's Adler-32 (yogo_amd/inflate.py) -- and one ``yogo_inflate_zlib`` launch
(yogo_amd/csrc/inflate.hip).  A chunk whose wrapper is not a plain zlib one is decoded on the host and copied as a raw row by
``yogo_blosc_lz4_decode``.  ``DEVICE_DECODE_ZLIB`` switches the route for this codec; it is off, because the host route measured
faster (profiles/zarr_feed.log).

Stacks compressed with Zstandard go to ``yogo_zstd_decode`` (yogo_amd/csrc/zstd.hip, yogo_amd/zstd.py) the same way: Blosc with
``cname="zstd"`` with one table row per Blosc block (one frame each; raw blocks and memcpyed chunks as raw rows), the ``zstd`` codec
with one row per chunk (``DEVICE_DECODE_ZSTD`` switches the route for this codec; it is off, because one serial chain per chunk
lost to the host there as it did for zlib: profiles/zstd_feed.log).  The frames go in one launch, the raw rows in
one ``yogo_blosc_lz4_decode`` launch behind it, as a zlib stack's do.  A chunk the device cannot take -- bit-shuffle,
``typesize > 1``, a stored size above the slot -- is decoded on the host and enters as raw rows.  The decoders' launch wrappers
and the iterator's skeleton are yogo_amd/device_decode.py's.

What differs between the four routes is one ``DeviceCodec`` record each in ``CODECS``, keyed by ``ZarrArray.device_codec``: how a
chunk's stored bytes become table entries (or that the chunk is the host's), the launch wrapper and its status texts, whether the
kernel copies raw rows itself, whether it takes a workspace, and which module constant switches the route.  Whether a row is raw
is carried beside the table (``BatchPlan.row_raw``), not in it: the fifth field is what the row's decoder reads there and nothing
else.  ``decode_rows`` makes the launches of a table -- for the feed, and for tools/bench_zarr_feed.py.
"""
from __future__ import annotations

import os
import threading
from collections import Counter
from concurrent.futures import Future, ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from yogo_amd import _hip, blosc, inflate, zstd
from yogo_amd.device_decode import ALIGN, MAX_THREADS, PrefetchFeed, center_crop_origin, decode_blocks, feed_device, gather, \
    inflate_streams, raise_first_bad, require_bytes, zstd_frames, zstd_work_bytes
from yogo_amd.zarr_store import ChunkTooLong, ZarrArray, ZarrGroup

RAW_PIECE = 1 << 16  # bytes of a raw block one wavefront of the device decoder copies (longer raw entries are cut up)
DEVICE_DECODE_ZLIB = False  # True: stacks under the zlib codec are inflated on the device.  Off: at batch 256 the device route feeds
#                             1.0-1.5 k img/s where the host's 16 threads feed 2.5-3.4 k (profiles/zarr_feed.log); PNG files do gain
DEVICE_DECODE_ZSTD = False  # True: stacks under the zstd codec (ONE frame, so one wavefront, per chunk) are decoded on the device.  Off: at
#                             batch 256 the device route feeds 2.5-3.6 k img/s of smooth-plus-noise frames where the host's 16 threads
#                             (libzstd) feed 3.6-5.4 k (profiles/zstd_feed.log); Blosc-zstd stacks, several frames per chunk, do gain

# one block of a stored chunk as its codec lists it: (src_off, src_len, dst_off, dst_len, the fifth field of the row its decoder reads
# -- a raw flag, an Adler-32 --, whether the bytes are raw: copied, not decoded), offsets relative to the chunk's stored / decoded start
Entry = Tuple[int, int, int, int, int, bool]


def _blosc_entries(takes: Callable[[int], bool]) -> Callable[[np.ndarray, int], Optional[List[Entry]]]:
    def entries(stored: np.ndarray, n: int) -> Optional[List[Entry]]:
        """one entry per Blosc block (a memcpyed chunk: one raw entry); None where the chunk's flags are not the decoder's"""
        flags, blocks = blosc.parse_chunk(stored, n)
        return [b + (bool(b[4]),) for b in blocks] if takes(flags) else None
    return entries


def _zlib_entries(stored: np.ndarray, n: int) -> Optional[List[Entry]]:
    """one stream per chunk, the fifth field its Adler-32; None where the wrapper is no plain zlib one: the host's to decode (or to refuse)"""
    try:
        off, ln, adler = inflate.split_zlib(stored)
    except ValueError:
        return None
    return [(off, ln, 0, n, adler, False)]


def _zstd_entries(stored: np.ndarray, n: int) -> Optional[List[Entry]]:
    """one frame per chunk"""
    return [(0, len(stored), 0, n, 0, False)]


@dataclass(frozen=True)
class DeviceCodec:
    """One device route of the feed; ``CODECS`` keys them by ``ZarrArray.device_codec``."""
    entries: Callable[[np.ndarray, int], Optional[List[Entry]]]   # (a chunk's stored bytes, chunk_nbytes) -> its blocks, or None: the
    #                                                                host decodes the chunk; ValueError for a malformed chunk
    launch: Callable[..., None]        # the decoder's launch wrapper (yogo_amd/device_decode.py)
    status: Mapping[int, str]          # its status texts
    copies_raw: bool = False           # its kernel copies raw rows itself, in the same launch; else they go to decode_blocks behind it
    workspace: bool = False            # the launch takes yogo_zstd_decode's workspace
    default_on: bool = True            # a store under this codec is decoded on the device unless the feed is told otherwise
    switch: Optional[str] = None       # the constant of this module that says so when a feed is built (tests and tools set it)

    def on(self) -> bool:
        return self.default_on if self.switch is None else bool(globals()[self.switch])


CODECS: Dict[str, DeviceCodec] = {
    "blosc": DeviceCodec(_blosc_entries(blosc.device_decodable), decode_blocks, blosc.LZ4_STATUS, copies_raw=True),
    "zlib": DeviceCodec(_zlib_entries, inflate_streams, inflate.INF_STATUS, default_on=DEVICE_DECODE_ZLIB, switch="DEVICE_DECODE_ZLIB"),
    "blosc-zstd": DeviceCodec(_blosc_entries(blosc.device_decodable_zstd), zstd_frames, zstd.ZSTD_STATUS, workspace=True),
    "zstd": DeviceCodec(_zstd_entries, zstd_frames, zstd.ZSTD_STATUS, workspace=True, default_on=DEVICE_DECODE_ZSTD, switch="DEVICE_DECODE_ZSTD"),
}


class FrameSource:
    """Where frame idx of a store lives: an [H, W, N] array (chunk (ty, tx, idx // cn), position idx % cn) or a group of 2-D
    arrays (member idx, chunk (ty, tx), position 0).  The members of a group must agree with member 0 in everything the
    kernel is told once per launch."""

    def __init__(self, root: Union[ZarrArray, ZarrGroup]):
        self.root = root
        if isinstance(root, ZarrArray):
            if root.ndim != 3:
                raise ValueError(f"zarr store {root.where}: an [H, W, N] array is expected, got shape {root.shape}")
            first, self.num_frames = root, root.shape[2]
        else:
            if len(root) == 0:
                raise ValueError(f"zarr store {root.where}: the group has no members")
            first, self.num_frames = root[0], len(root)
            if first.ndim != 2:
                raise ValueError(f"zarr store {first.where}: the members of the group must be 2-D, got shape {first.shape}")
        self.first = first
        self.H, self.W = first.shape[:2]
        self.ch, self.cw = first.chunks[:2]
        self.cn = first.chunks[2] if first.ndim == 3 else 1
        self.gh, self.gw = first.grid[:2]
        self.order_f = first.order == "F"
        self.fill = first.fill_value
        self.chunk_nbytes = first.chunk_nbytes
        self.chunk_stride = -(-self.chunk_nbytes // ALIGN) * ALIGN
        # room for one chunk's STORED bytes when they go to the device decoder: header, block starts and sizes of blocks of 64
        # bytes or more.  c-blosc writes no chunk above chunk_nbytes + 16 (it falls back to memcpyed); a longer one from
        # another writer (all blocks raw at a tiny blocksize) is decoded on the host instead.
        self.stored_stride = -(-(self.chunk_nbytes + blosc.HEADER + 8 * -(-self.chunk_nbytes // 64)) // ALIGN) * ALIGN

    def locate(self, idx: int) -> Tuple[ZarrArray, Optional[int], int]:
        """-> (array, its chunk coordinate on the frame axis or None for a 2-D member, position inside the chunk)"""
        if not 0 <= idx < self.num_frames:
            raise IndexError(f"frame {idx} is out of range for {self.num_frames} frames")
        if isinstance(self.root, ZarrArray):
            return self.root, idx // self.cn, idx % self.cn
        arr, f = self.root[idx], self.first
        if (arr.shape, arr.chunks, arr.order, arr.fill_value) != (f.shape, f.chunks, f.order, f.fill_value):
            raise RuntimeError(f"zarr store {arr.where}: shape {arr.shape} / chunks {arr.chunks} / order {arr.order} / fill "
                               f"{arr.fill_value} differ from member 0 ({f.shape} / {f.chunks} / {f.order} / {f.fill_value})")
        return arr, None, 0

    def max_chunks(self, batch_size: int) -> int:
        """the most chunks a batch of consecutive frames touches"""
        per_tile = batch_size if self.cn == 1 else min(batch_size, (batch_size + self.cn - 2) // self.cn + 1)
        return self.gh * self.gw * per_tile


@dataclass
class BatchPlan:
    """What frames [lo, hi) need: the distinct chunks present in the store, in staging order, and the kernel's tables."""
    lo: int
    hi: int
    keys: List[str]                       # store keys of the chunks to stage
    chunks: List[Tuple[ZarrArray, Tuple[int, ...]]]
    offsets: Dict[str, int]               # key -> byte offset in the staging buffer
    tile_off: np.ndarray                  # int64 [B, gh, gw], -1 where the key is absent from the store
    tile_k: np.ndarray                    # int32 [B]
    nbytes: int                           # bytes of the staging buffer in use
    stored: Optional[Dict[str, Tuple[int, List[Entry]]]] = None   # device decode: key -> (stored bytes, its block entries)
    row_chunk: Optional[List[int]] = None  # device decode: per row of the decoder's table, the index of its chunk in `keys`
    row_raw: Optional[np.ndarray] = None   # ... and whether the row is raw bytes (bool [rows])


def plan_batch(src: FrameSource, lo: int, hi: int) -> BatchPlan:
    B = hi - lo
    keys: List[str] = []
    chunks: List[Tuple[ZarrArray, Tuple[int, ...]]] = []
    offsets: Dict[str, int] = {}
    absent = set()
    tile_off = np.full((B, src.gh, src.gw), -1, dtype=np.int64)
    tile_k = np.zeros(B, dtype=np.int32)
    for b, idx in enumerate(range(lo, hi)):
        arr, tk, k = src.locate(idx)
        tile_k[b] = k
        for ty in range(src.gh):
            for tx in range(src.gw):
                coords = (ty, tx) if tk is None else (ty, tx, tk)
                key = arr.chunk_key(coords)
                if key in absent:
                    continue
                if key not in offsets:
                    if not arr.has_chunk(coords):
                        absent.add(key)
                        continue
                    offsets[key] = len(keys) * src.chunk_stride
                    keys.append(key)
                    chunks.append((arr, coords))
                tile_off[b, ty, tx] = offsets[key]
    return BatchPlan(lo, hi, keys, chunks, offsets, tile_off, tile_k, max(len(keys) * src.chunk_stride, ALIGN))


class ChunkStager:
    """Reads the chunks of a plan into a staging buffer on a thread pool (file reads and zlib release the GIL); one store
    handle per thread.  ``reads`` counts, per key, how often a chunk was read from the store."""

    def __init__(self, src: FrameSource, threads: Optional[int] = None):
        self.src = src
        self.threads = max(1, min(MAX_THREADS, threads or os.cpu_count() or 1))
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="zarr-read")
        self._local = threading.local()
        self._stores: List = []
        self._lock = threading.Lock()
        self.reads: Counter = Counter()

    def close(self) -> None:
        self._pool.shutdown(wait=True)
        with self._lock:
            for s in self._stores:
                s.close()
            self._stores.clear()

    def _store(self, arr: ZarrArray):
        """this thread's handle of the store"""
        store = getattr(self._local, "store", None)
        if store is None:
            store = self._local.store = arr.store.clone()
            with self._lock:
                self._stores.append(store)
        return store

    def _read(self, arr: ZarrArray, coords: Tuple[int, ...], out: np.ndarray) -> None:
        store = self._store(arr)
        try:
            arr.with_store(store).read_chunk_into(coords, out)
        except KeyError:
            raise RuntimeError(f"zarr store {arr.where}: chunk {arr.chunk_key(coords)!r} disappeared from the store") from None

    def stage(self, plan: BatchPlan, buf: np.ndarray, prev: Optional[Tuple[BatchPlan, np.ndarray]] = None) -> None:
        """every chunk of ``plan`` at its offset in ``buf``; a chunk that ``prev`` (the previous plan and its filled buffer)
        holds is copied from there.  Raises the first chunk's RuntimeError after every read has ended."""
        n = self.src.chunk_nbytes
        futures: List[Future] = []
        for key, (arr, coords) in zip(plan.keys, plan.chunks):
            off = plan.offsets[key]
            if prev is not None and key in prev[0].offsets:
                poff = prev[0].offsets[key]
                buf[off:off + n] = prev[1][poff:poff + n]
                continue
            self.reads[key] += 1
            futures.append(self._pool.submit(self._read, arr, coords, buf[off:off + n]))
        gather(futures)

    def _read_stored(self, arr: ZarrArray, coords: Tuple[int, ...], out: np.ndarray) -> Tuple[int, List[Entry]]:
        """the stored bytes of one chunk into ``out`` (stored_stride bytes) -> (bytes in use, block entries relative to the chunk).
        What the device cannot decode is decoded here and becomes one raw entry."""
        n = self.src.chunk_nbytes
        key = arr.chunk_key(coords)
        store = self._store(arr)
        a = arr.with_store(store)
        name = self.src.first.device_codec   # the table's rows are read by the STORE's decoder: a group member under another
        try:                                  # compressor than member 0's is decoded on the host, as before
            if name is not None and a.device_codec == name:
                try:
                    got = a.read_stored_into(coords, out)
                    entries = CODECS[name].entries(out[:got], n)
                    if entries is not None:
                        return got, entries
                except (ChunkTooLong, NotImplementedError):
                    pass
                except ValueError as e:
                    raise RuntimeError(f"zarr store {arr.where}: chunk {key!r} could not be decoded ({type(e).__name__}: {e})") from e
            a.read_chunk_into(coords, out[:n])
            return n, [(0, n, 0, n, 1, True)]
        except KeyError:
            raise RuntimeError(f"zarr store {arr.where}: chunk {key!r} disappeared from the store") from None

    def stage_stored(self, plan: BatchPlan, buf: np.ndarray, prev: Optional[Tuple[BatchPlan, np.ndarray]] = None) -> np.ndarray:
        """(device decode) the STORED bytes of every chunk of ``plan`` at ``i * stored_stride`` in ``buf``; fills ``plan.stored``
        and returns the decoder's table, int64 [rows, 5]: (src_off, src_len, dst_off, dst_len, fifth) with dst_off in the layout of
        ``plan.offsets``; fifth: what the row's decoder reads there -- the raw flag (1 for every raw row), a zlib stream's Adler-32.
        ``plan.row_chunk`` / ``plan.row_raw`` say per row which chunk it belongs to and whether it is raw.  The rows are in the
        order ``decode_rows`` launches them in: under a codec whose kernel does not copy raw rows, those come last.  Chunks that
        ``prev`` holds are copied from there; errors as in ``stage``."""
        stride = self.src.stored_stride
        plan.stored = {}
        pending: Dict[str, Future] = {}
        for i, (key, (arr, coords)) in enumerate(zip(plan.keys, plan.chunks)):
            soff = i * stride
            if prev is not None and prev[0].stored and key in prev[0].stored:
                used, entries = prev[0].stored[key]
                poff = prev[0].keys.index(key) * stride
                buf[soff:soff + used] = prev[1][poff:poff + used]
                plan.stored[key] = (used, entries)
                continue
            self.reads[key] += 1
            pending[key] = self._pool.submit(self._read_stored, arr, coords, buf[soff:soff + stride])
        plan.stored.update(zip(pending, gather(list(pending.values()))))
        rows, owner = [], []
        for i, key in enumerate(plan.keys):
            for so, sl, do, dl, fifth, raw in plan.stored[key][1]:
                # a long raw entry (a memcpyed chunk, a chunk decoded on the host) goes to several wavefronts
                for at in (range(0, sl, RAW_PIECE) if raw else (0,)):
                    ln = min(RAW_PIECE, sl - at) if raw else sl
                    rows.append((i * stride + so + at, ln, plan.offsets[key] + do + at, ln if raw else dl, fifth, raw))
                    owner.append(i)
        table = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
        if not CODECS[self.src.first.device_codec].copies_raw:
            order = np.argsort(table[:, 5], kind="stable")
            table, owner = table[order], [owner[i] for i in order]
        plan.row_chunk, plan.row_raw = owner, table[:, 5] != 0
        return np.ascontiguousarray(table[:, :5])


def decode_rows(codec: DeviceCodec, stored: torch.Tensor, table: torch.Tensor, raw: np.ndarray, out: torch.Tensor, status: torch.Tensor,
                work: Optional[torch.Tensor] = None) -> int:
    """(current stream) the rows of ``ChunkStager.stage_stored`` decoded from ``stored`` into ``out``: table int64 [rows, 5] and
    status int32 [rows] on the device, raw bool [rows] on the host (``plan.row_raw``).  Either the codec's kernel over all rows in
    one launch, or -- a kernel that does not copy raw rows -- over the coded rows, and ``yogo_blosc_lz4_decode`` over the raw ones
    behind them.  work: the workspace of a codec that takes one, ``zstd_work_bytes`` of the coded rows.  -> how many rows the
    first launch took"""
    first = len(raw) if codec.copies_raw else len(raw) - int(np.count_nonzero(raw))
    if not codec.copies_raw and raw[:first].any():
        raise ValueError("decode_rows: a raw row lies before a coded one")
    if first:
        codec.launch(stored, table[:first], out, status[:first], *((work,) if codec.workspace else ()))
    if first < len(raw):
        decode_blocks(stored, table[first:], out, status[first:])
    return first


def unpack(staged: torch.Tensor, tile_off: np.ndarray, tile_k: np.ndarray, *, chunks: Sequence[int], order_f: bool, fill: int,
           frame_shape: Tuple[int, int], out: torch.Tensor, top: int = 0, left: int = 0,
           tile_off_dev: Optional[torch.Tensor] = None, tile_k_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``yogo_zarr_unpack`` launch on the current stream.  staged: 1-D uint8 device tensor of decoded chunks; tile_off
    [B, gh, gw] / tile_k [B]: the host tables (checked here: the kernel trusts them), optionally with their device copies;
    out: contiguous [B, 1, OH, OW] uint8 or float32 on the same device."""
    _hip.require_cuda(staged, "the staged zarr chunks")
    _hip.require_cuda(out, "the unpack output")
    ch, cw, cn = (int(v) for v in chunks)
    H, W = (int(v) for v in frame_shape)
    require_bytes("unpack", "staged", staged)
    if out.dtype not in (torch.uint8, torch.float32) or out.ndim != 4 or out.shape[1] != 1 or not out.is_contiguous():
        raise ValueError(f"unpack: out must be a contiguous [B, 1, OH, OW] uint8 or float32 tensor, got {tuple(out.shape)} {out.dtype}")
    if out.device != staged.device:
        raise ValueError(f"unpack: the chunks are on {staged.device}, out on {out.device}")
    B, _, OH, OW = (int(v) for v in out.shape)
    gh, gw = -(-H // ch), -(-W // cw)
    toff = np.ascontiguousarray(tile_off, dtype=np.int64)
    tk = np.ascontiguousarray(tile_k, dtype=np.int32)
    if toff.shape != (B, gh, gw) or tk.shape != (B,):
        raise ValueError(f"unpack: tile_off {toff.shape} / tile_k {tk.shape} for {B} rows of a {gh} x {gw} tile grid")
    if B == 0:
        return out
    if int(tk.min()) < 0 or int(tk.max()) >= cn:
        raise IndexError(f"unpack: tile_k outside [0, {cn})")
    used = toff[toff >= 0]
    if used.size and (int((used % 16).max()) != 0 or int(used.max()) + ch * cw * cn > staged.numel()):
        raise IndexError(f"unpack: a tile offset is not 16-byte aligned or its chunk ends after the {staged.numel()} staged bytes")
    dev = out.device
    if tile_off_dev is None:
        tile_off_dev = torch.from_numpy(toff).to(dev)
    if tile_k_dev is None:
        tile_k_dev = torch.from_numpy(tk).to(dev)
    with torch.cuda.device(dev):
        _hip.call("yogo_zarr_unpack", staged, staged.numel(), tile_off_dev, tile_k_dev, B, gh, gw, ch, cw, cn, 1 if order_f else 0,
                  int(fill), H, W, int(top), int(left), OH, OW, out, 1 if out.dtype == torch.float32 else 0, _hip.stream_ptr())
    return out


class ZarrDeviceFeed(PrefetchFeed):
    """Iterator over ``(device batch [B, 1, OH, OW], names)`` in index order; the last batch may be partial; a batch that raises
    RuntimeError (an unreadable chunk) costs that batch alone (device_decode.PrefetchFeed).  ``crop``: (OH, OW) of a centre crop
    done in the kernel; ``normalize``: fp32 ``/ 255`` in the kernel, else uint8.
    ``num_frames``: how many frames to walk (default: ``len(dataset)``, as the reference's DataLoader does, and never more
    than the stack holds).  ``device_decode``: a Blosc stack with LZ4 or zstd blocks (and, with DEVICE_DECODE_ZLIB / DEVICE_DECODE_ZSTD set, a zlib / zstd stack) is decoded on the device
    (module docstring); False takes the host route (A/B runs); every other source takes the host route whatever it says."""

    def __init__(self, dataset, batch_size: int, device, crop: Optional[Tuple[int, int]] = None, normalize: bool = False,
                 num_frames: Optional[int] = None, device_decode: bool = True):
        dev = feed_device(device, batch_size, "the zarr feed unpacks")
        self.dataset, self.batch_size, self.device, self.normalize = dataset, int(batch_size), dev, bool(normalize)
        self.src = src = FrameSource(dataset.zarr_store)
        n = min(len(dataset) if num_frames is None else int(num_frames), src.num_frames)
        self.num_frames = n
        self.OH, self.OW = (src.H, src.W) if crop is None else (int(crop[0]), int(crop[1]))
        self.top, self.left = center_crop_origin(src.H, src.W, self.OH, self.OW)
        cap = max(ALIGN, src.max_chunks(self.batch_size) * src.chunk_stride)
        self._pinned = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._host = [p.numpy() for p in self._pinned]
        self._dev = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.codec = src.first.device_codec
        self.route = CODECS.get(self.codec)
        self.device_decode = bool(device_decode) and self.route is not None and self.route.on()
        self._zwork: Optional[torch.Tensor] = None   # yogo_zstd_decode's workspace
        if self.device_decode:
            scap = src.max_chunks(self.batch_size) * src.stored_stride
            self._spinned = [torch.empty(scap, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self._shost = [p.numpy() for p in self._spinned]
            self._sdev = [torch.empty(scap, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._side = torch.cuda.Stream(dev)
        self._uploaded: List[Optional[torch.cuda.Event]] = [None, None]   # slot's pinned buffer may be overwritten after this
        self._consumed: List[Optional[torch.cuda.Event]] = [None, None]   # slot's device buffer may be overwritten after this
        self._last: Optional[Tuple[int, BatchPlan, np.ndarray]] = None   # the batch staged last, its plan and its filled host buffer
        self.stager = ChunkStager(src)
        super().__init__(n, self.batch_size, "zarr-feed")

    def close(self) -> None:
        super().close()
        self.stager.close()

    def _upload_stored(self, plan: BatchPlan, slot: int) -> None:
        """(side stream) the stored bytes in use; neighbours whose gap is under a quarter of a chunk's room travel in one copy"""
        stride = self.src.stored_stride
        runs: List[List[int]] = []
        for i, key in enumerate(plan.keys):
            a, b = i * stride, i * stride + plan.stored[key][0]
            if runs and a - runs[-1][1] <= stride // 4:
                runs[-1][1] = b
            else:
                runs.append([a, b])
        for a, b in runs:
            self._sdev[slot][a:b].copy_(self._spinned[slot][a:b], non_blocking=True)

    def _decode(self, plan: BatchPlan, table: np.ndarray, slot: int) -> Tuple[Optional[torch.Tensor], int]:
        """(side stream) stored bytes and table up, the rows decoded into the slot's device buffer (``decode_rows``: one launch, and
        one of the raw rows -- raw blocks, memcpyed and host-decoded chunks -- where the codec's kernel does not copy them)
        -> (the per-row status, None without a launch; how many rows the first launch took)"""
        if not len(table):
            return None, 0
        self._upload_stored(plan, slot)
        coded = len(table) - int(np.count_nonzero(plan.row_raw))
        if self.route.workspace and coded and (self._zwork is None or self._zwork.numel() < zstd_work_bytes(coded)):
            self._zwork = torch.empty(zstd_work_bytes(coded), dtype=torch.uint8, device=self.device)   # (grows; the launches of both
            #                                                                     slots run on the side stream, in order)
        status = torch.empty(len(table), dtype=torch.int32, device=self.device)
        first = decode_rows(self.route, self._sdev[slot], torch.from_numpy(table).to(self.device), plan.row_raw, self._dev[slot], status,
                            self._zwork)
        return status, first

    def _load(self, n: int):
        """(loader thread) stage batch n and start its upload on the side stream; through the device decoder: the stored bytes are
        staged and decoded there, then the per-row status comes back -- RuntimeError naming the first bad chunk"""
        slot = n % 2
        lo, hi = self.batches[n]
        plan = plan_batch(self.src, lo, hi)
        if self._uploaded[slot] is not None:
            self._uploaded[slot].synchronize()
        host = (self._shost if self.device_decode else self._host)[slot]
        prev = (self._last[1], self._last[2]) if self._last is not None and self._last[0] == n - 1 else None
        self._last = None
        table = self.stager.stage_stored(plan, host, prev) if self.device_decode else self.stager.stage(plan, host, prev)
        self._last = (n, plan, host)
        with torch.cuda.device(self.device), torch.cuda.stream(self._side):
            if self._consumed[slot] is not None:
                self._side.wait_event(self._consumed[slot])
            toff = torch.from_numpy(plan.tile_off).to(self.device)
            tk = torch.from_numpy(plan.tile_k).to(self.device)
            if self.device_decode:
                status, n_inflate = self._decode(plan, table, slot)
            else:
                status, n_inflate = None, 0
                self._dev[slot][:plan.nbytes].copy_(self._pinned[slot][:plan.nbytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._side)
            bad = status.cpu() if status is not None else None   # waits for the decode: this thread overlaps the consumer already
        self._uploaded[slot] = ev
        if bad is not None and bool(bad.any()):
            self._last = None   # what a bad chunk left in the device buffer is not handed on
            names = [f"zarr store {plan.chunks[i][0].where}: chunk {plan.keys[i]!r}" for i in plan.row_chunk]
            raise_first_bad(bad[:n_inflate], self.route.status, names.__getitem__)
            raise_first_bad(bad[n_inflate:], blosc.LZ4_STATUS, names[n_inflate:].__getitem__)
        return plan, toff, tk, ev

    def _deliver(self, n: int, loaded) -> Tuple[torch.Tensor, Tuple[str, ...]]:
        """(caller's thread) the unpack launch on the current stream, behind the upload"""
        plan, toff, tk, ev = loaded
        slot = n % 2
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            toff.record_stream(cur)
            tk.record_stream(cur)
            out = torch.empty((plan.hi - plan.lo, 1, self.OH, self.OW), dtype=torch.float32 if self.normalize else torch.uint8,
                              device=self.device)
            unpack(self._dev[slot][:plan.nbytes], plan.tile_off, plan.tile_k, chunks=(self.src.ch, self.src.cw, self.src.cn),
                   order_f=self.src.order_f, fill=self.src.fill, frame_shape=(self.src.H, self.src.W), out=out, top=self.top,
                   left=self.left, tile_off_dev=toff, tile_k_dev=tk)
            done = torch.cuda.Event()
            done.record(cur)
        self._consumed[slot] = done
        return out, tuple(self.dataset.image_name_from_idx(i) for i in range(plan.lo, plan.hi))
