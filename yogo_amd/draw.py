"""``predict(..., draw_boxes=True, device_draw=True)`` / ``yogo infer --draw-boxes --device-draw``: the boxes are drawn and the PNG
files encoded on the device.

The host route (``yogo_amd.utils.utils.draw_yogo_prediction``) copies every image and its decoded predictions to the host, draws
with PIL -- one ``rectangle`` and one ``text`` call per box -- and saves with ``compress_level=1``.  Here one launch of
``yogo_draw_boxes`` (yogo_amd/csrc/draw_boxes.hip) renders the RGBA frames of a whole batch from the kept rows of
``format_preds_batched``, one launch of ``yogo_png_encode`` (yogo_amd/csrc/png_encode.hip, restated in yogo_amd/png_encode.py)
turns them into files, and the host reads the finished bytes and writes them on a small pool of threads.  The promise is the same
PIXELS: a file of this route decodes to exactly the RGBA array the host route's file decodes to; its bytes are compressed differently.

What stays on the host, once per run: the colour table (``bbox_colour``) and the glyph atlas.  The atlas is PIL's own rendering of
every class label -- ``ImageDraw.Draw(...).getfont()`` and ``font.getmask2(label, "L", start=(fx, fy))``, what ``ImageDraw.text``
draws with -- at every sub-pixel phase that changes it.  FreeType's masks depend on the fraction of the text position only through a
few intervals per axis; their edges are found per label and axis by bisection over fp32 values (the fraction of an fp32 coordinate is
exact in fp32, so a cut is the first float of the new interval) and the kernel picks the variant by comparing the fraction to them.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from yogo_amd.utils.utils import bbox_colour

MAX_WRITERS = 8            # file writes: a small fixed pool, never sized from the machine's CPU count
_SCAN_STEPS = 32           # the fractions (-1, 1) are scanned at this many points per unit before the bisection
_OTHER_AXIS = (-0.75, -0.25, 0.25, 0.75)   # the other axis' fraction while one axis is scanned


def check_labels(labels: Sequence[str]) -> None:
    for name in labels:
        if "\n" in name or "\r" in name:
            raise ValueError(f"device_draw: the class name {name!r} contains a line break; PIL lays such text out as several lines, "
                             "which the device route does not do")


def colour_table(num_classes: int, num_channels: int) -> np.ndarray:
    """[C, 4] uint8: ``bbox_colour(class, num_channels - 5)``, the class count the host route passes (kept on purpose)"""
    return np.asarray([bbox_colour(c, num_channels - 5) for c in range(num_classes)], dtype=np.uint8).reshape(num_classes, 4)


def default_font():
    import PIL.Image
    import PIL.ImageDraw

    return PIL.ImageDraw.Draw(PIL.Image.new("RGBA", (1, 1))).getfont()


def render_mask(font, label: str, fx: float, fy: float) -> Tuple[int, int, int, int, bytes]:
    """(width, height, offset x, offset y, bytes) of the mask ``ImageDraw.text`` blends for `label` at the fractions (fx, fy)"""
    if hasattr(font, "getmask2"):
        mask, offset = font.getmask2(label, "L", start=(float(fx), float(fy)))
    else:   # a bitmap font (no FreeType): one mask, no offset
        mask, offset = font.getmask(label, "L"), (0, 0)
    w, h = mask.size
    return int(w), int(h), int(offset[0]), int(offset[1]), (bytes(mask) if w and h else b"")


def _axis_cuts(font, label: str, axis: int) -> np.ndarray:
    """the fp32 fractions in (-1, 1) at which the mask of `label` changes along `axis`, each the FIRST value of its interval"""
    memo: Dict[float, tuple] = {}

    def key(t: np.float32):
        t = float(t)
        if t not in memo:
            memo[t] = tuple(render_mask(font, label, *((t, s) if axis == 0 else (s, t))) for s in _OTHER_AXIS)
        return memo[t]

    one = np.float32(1.0)
    grid = [np.nextafter(-one, np.float32(0))] + [np.float32(i / _SCAN_STEPS) for i in range(-_SCAN_STEPS + 1, _SCAN_STEPS)]
    grid.append(np.nextafter(one, np.float32(0)))
    cuts = []
    for lo, hi in zip(grid[:-1], grid[1:]):
        if key(lo) == key(hi):
            continue
        klo = key(lo)
        while np.nextafter(lo, hi) != hi:
            mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
            if key(mid) == klo:
                lo = mid
            else:
                hi = mid
        cuts.append(hi)
    return np.asarray(cuts, dtype=np.float32)


class GlyphAtlas:
    """Every label's mask variants.  ``lookup(label, fx, fy)`` is the selection rule of the kernel: the variant index along an axis
    is the number of cuts at or below the fraction."""

    def __init__(self, labels: Sequence[str], font=None) -> None:
        check_labels(labels)
        self.labels = list(labels)
        self.font = font if font is not None else default_font()
        self.xcuts: List[np.ndarray] = []
        self.ycuts: List[np.ndarray] = []
        self.variants: List[List[List[Tuple[int, int, int, int, bytes]]]] = []   # [label][ix][iy]
        has_phase = hasattr(self.font, "getmask2")
        for label in self.labels:
            xc = _axis_cuts(self.font, label, 0) if has_phase else np.zeros(0, dtype=np.float32)
            yc = _axis_cuts(self.font, label, 1) if has_phase else np.zeros(0, dtype=np.float32)
            self.xcuts.append(xc)
            self.ycuts.append(yc)
            xs, ys = self._midpoints(xc), self._midpoints(yc)
            self.variants.append([[render_mask(self.font, label, fx, fy) for fy in ys] for fx in xs])

    @staticmethod
    def _midpoints(cuts: np.ndarray) -> List[float]:
        edges = [-1.0] + [float(c) for c in cuts] + [1.0]
        return [float(np.float32((a + b) / 2)) for a, b in zip(edges[:-1], edges[1:])]

    def lookup(self, label: int, fx: float, fy: float) -> Tuple[int, int, int, int, bytes]:
        ix = int(np.count_nonzero(self.xcuts[label] <= np.float32(fx)))
        iy = int(np.count_nonzero(self.ycuts[label] <= np.float32(fy)))
        return self.variants[label][ix][iy]

    def tables(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(label_meta int32 [C, 6] = x-cut offset, x cuts, y-cut offset, y cuts, first variant, 0; cuts float32; variants int32
        [n, 5] = width, height, offset x, offset y, byte offset; glyph bytes uint8): what ``yogo_draw_boxes`` takes; variant
        (ix, iy) of a label is row ``first + ix * (y cuts + 1) + iy``"""
        meta, cuts, var, blob = [], [], [], bytearray()
        for xc, yc, grid in zip(self.xcuts, self.ycuts, self.variants):
            meta.append([len(cuts), len(xc), len(cuts) + len(xc), len(yc), len(var), 0])
            cuts.extend(xc.tolist())
            cuts.extend(yc.tolist())
            for col in grid:
                for w, h, ox, oy, data in col:
                    var.append([w, h, ox, oy, len(blob)])
                    blob += data
        return (np.asarray(meta, dtype=np.int32).reshape(len(self.labels), 6), np.asarray(cuts + [0.0], dtype=np.float32),
                np.asarray(var, dtype=np.int32).reshape(len(var), 5), np.frombuffer(bytes(blob) + b"\x00", dtype=np.uint8).copy())


class DeviceAtlas:
    """the atlas and the colour table in device memory"""

    def __init__(self, atlas: GlyphAtlas, num_channels: int, device) -> None:
        meta, cuts, var, blob = atlas.tables()
        self.num_classes = len(atlas.labels)
        self.n_cuts, self.n_variants, self.glyph_bytes = len(cuts) - 1, len(var), len(blob) - 1
        self.meta = torch.from_numpy(meta).to(device)
        self.cuts = torch.from_numpy(cuts).to(device)
        self.var = torch.from_numpy(var if len(var) else np.zeros((1, 5), dtype=np.int32)).to(device)
        self.blob = torch.from_numpy(blob).to(device)
        self.colours = torch.from_numpy(colour_table(self.num_classes, num_channels)).to(device)


def render_boxes(images: torch.Tensor, rows: torch.Tensor, counts: torch.Tensor, atlas: DeviceAtlas, normalised: bool,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """images [B, 1|3, H, W] uint8 or float32 on the device, the kept rows [B, cap, 5+C] (xyxy) and counts [B] of
    ``format_preds_batched`` -> [B, H, W, 4] uint8 RGBA: what ``draw_yogo_prediction`` draws, pixel for pixel.  One launch."""
    from yogo_amd import _hip

    _hip.require_cuda(images, "the images to draw on")
    _hip.require_cuda(rows, "the kept rows")
    if images.ndim != 4 or images.shape[1] not in (1, 3) or images.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"images must be uint8 or float32 [B, 1|3, H, W], got {images.dtype} {tuple(images.shape)}")
    B, Cimg, H, W = (int(v) for v in images.shape)
    if rows.ndim != 3 or rows.shape[0] != B or rows.dtype != torch.float32 or rows.shape[2] != 5 + atlas.num_classes:
        raise ValueError(f"rows must be float32 [{B}, cap, {5 + atlas.num_classes}], got {rows.dtype} {tuple(rows.shape)}")
    if counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
        raise ValueError(f"counts must be int32 [{B}], got {counts.dtype} {tuple(counts.shape)}")
    images, rows, counts = images.contiguous(), rows.contiguous(), counts.contiguous()
    if out is None:
        out = torch.empty(B, H, W, 4, dtype=torch.uint8, device=images.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, 4) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"out must be a contiguous uint8 [{B}, {H}, {W}, 4] on the device")
    if B == 0:
        return out
    with torch.cuda.device(images.device):
        _hip.call("yogo_draw_boxes", images, int(images.dtype == torch.float32), int(bool(normalised)), B, Cimg, H, W, rows, counts,
                  int(rows.shape[1]), int(rows.shape[2]), atlas.colours, atlas.meta, atlas.cuts, atlas.n_cuts, atlas.var, atlas.n_variants,
                  atlas.blob, atlas.glyph_bytes, out, _hip.stream_ptr())
    return out


def check_level(level) -> int:
    from yogo_amd.png_encode import LEVELS

    if isinstance(level, bool) or not isinstance(level, int) or level not in LEVELS:
        raise ValueError(f"the PNG encoder's level must be one of {LEVELS} (0: literals only, 1: literals and matches), got {level!r}")
    return level


def encode_bound(H: int, W: int, bpp: int = 4, level: int = 0) -> Tuple[int, int]:
    """(bytes of a file slot, bytes of work space per image) of ``yogo_png_encode_level`` (``yogo_png_encode_bound_level``; runs on
    the host).  The slot is the same at every level; level 1 keeps a band's filtered bytes and tokens in the work space."""
    import ctypes

    from yogo_amd import _hip

    slot, work = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _hip.call("yogo_png_encode_bound_level", int(H), int(W), int(bpp), check_level(level), ctypes.addressof(slot), ctypes.addressof(work))
    return int(slot.value), int(work.value)


def encode_png(pixels: torch.Tensor, files: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None, packed: bool = False,
               slot_bytes: Optional[int] = None, level: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """pixels [B, H, W, bpp] uint8 on the device -> (files uint8, offsets int64 [B + 1], status int32 [B]).  File b is
    ``files[offsets[b]: offsets[b + 1]]`` when `packed`, else ``files[b * slot: b * slot + offsets[b + 1] - offsets[b]]`` in its own
    slot of `slot_bytes` (default: the bound); a nonzero status means the image has no file (length 0).  `level` 0 codes literals
    only, 1 literals and matches (yogo_amd/png_encode.py); the work space is sized by it.  Two launches: the bands, then the assembly."""
    from yogo_amd import _hip

    _hip.require_cuda(pixels, "the pixels to encode")
    if pixels.ndim != 4 or pixels.dtype != torch.uint8 or not 1 <= pixels.shape[3] <= 4 or not pixels.is_contiguous():
        raise ValueError(f"pixels must be contiguous uint8 [B, H, W, 1 .. 4], got {pixels.dtype} {tuple(pixels.shape)}")
    B, H, W, bpp = (int(v) for v in pixels.shape)
    bound, work_per = encode_bound(H, W, bpp, level)
    slot = bound if slot_bytes is None else int(slot_bytes)
    dev = pixels.device
    if files is None:
        files = torch.empty(max(B * slot, 1), dtype=torch.uint8, device=dev)
    if work is None:
        work = torch.empty(max(B * work_per, 16), dtype=torch.uint8, device=dev)
    if files.numel() < B * slot or work.numel() < B * work_per:
        raise ValueError(f"encode_png: {B} images need {B * slot} bytes of files and {B * work_per} of work space at level {level}")
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    status = torch.empty(max(B, 1), dtype=torch.int32, device=dev)[:B]
    if B:
        with torch.cuda.device(dev):
            _hip.call("yogo_png_encode_level", pixels, B, H, W, bpp, level, files, slot, int(bool(packed)), offsets, status, work,
                      int(work.numel()), _hip.stream_ptr())
    else:
        offsets.zero_()
    return files, offsets, status


def _write(path: Path, data) -> None:
    with open(path, "wb") as f:
        f.write(data)


def _save_pil(path: Path, rgba: np.ndarray) -> None:
    import PIL.Image

    PIL.Image.fromarray(rgba, mode="RGBA").save(path, compress_level=1)


class DrawSink:
    """Owns what a batch of drawn images needs -- the RGBA frames, the file slots, the encoder's work space, the writer pool -- and
    reuses it from batch to batch.  The buffers are allocated at the first batch for its size (B frames of 4 H W bytes, B slots of
    about as many and as much work space again: at 772 x 1032 and B = 256 three times 0.8 GB; at `level` 1 the work space is four
    times that, 3.3 GB) and are kept until ``close()``."""

    def __init__(self, device, labels: Sequence[str], normalised: bool, output_dir, filetype: str = ".png", level: int = 0) -> None:
        self.level = check_level(level)
        if self.level and filetype != ".png":
            raise ValueError(f"level {level} is the PNG encoder's: nothing is encoded for {filetype} files")
        self.device = torch.device(device)
        self.glyphs = GlyphAtlas(labels)
        self.atlas: Optional[DeviceAtlas] = None   # uploaded at the first batch: the colours depend on its channel count
        self.channels = 0
        self.normalised, self.output_dir, self.filetype = bool(normalised), Path(output_dir), filetype
        self.rgba: Optional[torch.Tensor] = None
        self.files: Optional[torch.Tensor] = None
        self.work: Optional[torch.Tensor] = None
        self.pool = ThreadPoolExecutor(max_workers=MAX_WRITERS)
        self.pending: list = []

    def _buffers(self, B: int, H: int, W: int) -> None:
        if self.rgba is None or self.rgba.shape[0] < B or tuple(self.rgba.shape[1:3]) != (H, W):
            self.rgba = torch.empty(B, H, W, 4, dtype=torch.uint8, device=self.device)
            if self.filetype == ".png":
                slot, work = encode_bound(H, W, 4, self.level)
                self.files = torch.empty(B * slot, dtype=torch.uint8, device=self.device)
                self.work = torch.empty(B * work, dtype=torch.uint8, device=self.device)

    def _wait(self) -> None:
        for f in self.pending:
            f.result()
        self.pending.clear()

    def submit(self, images: torch.Tensor, rows: torch.Tensor, counts: torch.Tensor, fnames) -> None:
        """draw, encode, read back and hand the files of one batch to the writers"""
        B, channels, H, W = (int(v) for v in images.shape)
        if self.atlas is None or channels != self.channels:
            self.atlas, self.channels = DeviceAtlas(self.glyphs, channels, self.device), channels
        self._buffers(B, H, W)
        rgba = render_boxes(images, rows, counts, self.atlas, self.normalised, out=self.rgba[:B])
        paths = [self.output_dir / Path(f).with_suffix(self.filetype).name for f in fnames]
        if self.filetype != ".png":   # nothing to encode in an uncompressed TIFF: the draw is the device's, the file PIL's
            host = rgba.cpu().numpy()
            self._wait()
            self.pending = [self.pool.submit(_save_pil, p, host[k]) for k, p in enumerate(paths)]
            return
        _, offsets, status = encode_png(rgba, self.files, self.work, packed=True, level=self.level)
        head = torch.cat([offsets, status.to(torch.int64)]).cpu().numpy()
        off, st = head[: B + 1], head[B + 1:]
        data = self.files[: int(off[B])].cpu().numpy()
        self._wait()   # (the previous batch's writes ran under this batch's launches)
        view = memoryview(data)
        for k, p in enumerate(paths):
            if st[k]:   # the encoder gave this image up: PIL encodes it from the pixels
                self.pending.append(self.pool.submit(_save_pil, p, rgba[k].cpu().numpy()))
            else:
                self.pending.append(self.pool.submit(_write, p, view[int(off[k]): int(off[k + 1])]))

    def close(self) -> None:
        try:
            self._wait()
        finally:
            self.pool.shutdown(wait=True)
            self.rgba = self.files = self.work = None
