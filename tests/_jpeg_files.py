"""JPEG files for the tests of yogo_amd/jpeg.py and yogo_jpeg_decode, written by PIL at test time: the grid of formats, sizes,
qualities, contents and writer options, and the corrupted set (truncations and seeded single-byte changes)."""
import io
import warnings

import numpy as np
from PIL import Image

FORMATS = ("grey", "444", "422", "420")
SIZES = ((1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (35, 37), (64, 129))   # (H, W)
QUALITIES = (30, 75, 95, 100)
CONTENTS = ("noise", "ramp", "zero", "full", "checker")
OPTIONS = ({}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1})
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def content(kind: str, H: int, W: int, planes: int, rng) -> np.ndarray:
    """uint8 [H, W, planes]"""
    if kind == "noise":
        a = rng.integers(0, 256, (H, W, planes))
    elif kind == "ramp":
        yy, xx = np.mgrid[0:H, 0:W]
        a = (yy * 3 + xx * 2)[..., None] + np.arange(planes) * 40 + rng.integers(-6, 7, (H, W, planes))
    elif kind == "zero":
        a = np.zeros((H, W, planes))
    elif kind == "full":
        a = np.full((H, W, planes), 255)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.repeat((((yy + xx) & 1) * 255)[..., None], planes, axis=2)
    return np.clip(a, 0, 255).astype(np.uint8)


def write(fmt: str, H: int, W: int, quality: int, kind: str, rng, **options) -> bytes:
    """one file's bytes"""
    a = content(kind, H, W, 1 if fmt == "grey" else 3, rng)
    im = Image.fromarray(a[..., 0], "L") if fmt == "grey" else Image.fromarray(a, "RGB")
    buf = io.BytesIO()
    kw = {} if fmt == "grey" else {"subsampling": SUBSAMPLING[fmt]}
    im.save(buf, format="JPEG", quality=quality, **kw, **options)
    return buf.getvalue()


def pil_pixels(data: bytes, rgb: bool):
    """what ``read_image`` gives of the bytes: uint8 [1 | 3, H, W]; None where PIL raises or warns"""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with Image.open(io.BytesIO(data)) as im:
                a = np.asarray(im.convert("RGB" if rgb else "L"), dtype=np.uint8)
    except Exception:
        return None
    return np.ascontiguousarray(a.transpose(2, 0, 1)) if rgb else a[None].copy()


def grid():
    """every case of the grid: (name, bytes), the seed a function of the case"""
    for fi, fmt in enumerate(FORMATS):
        for H, W in SIZES:
            for quality in QUALITIES:
                for ki, kind in enumerate(CONTENTS):
                    for oi, options in enumerate(OPTIONS):
                        rng = np.random.default_rng(((fi * 200 + H) * 200 + W) * 100 + quality + ki)
                        yield f"{fmt}-{H}x{W}-q{quality}-{kind}-o{oi}", write(fmt, H, W, quality, kind, rng, **options)


def corrupted(seed: int = 0):
    """the corrupted set: 35 x 37 files, grey and 4:2:0, with and without restart markers; each truncated at 16 evenly spread
    lengths and with 200 seeded single-byte changes across header and scan -> (name, bytes)"""
    rng = np.random.default_rng(seed)
    for fmt in ("grey", "420"):
        for oi, options in enumerate(({}, {"restart_marker_blocks": 3})):
            data = write(fmt, 35, 37, 75, "ramp", np.random.default_rng(7), **options)
            for k in range(16):
                yield f"{fmt}-o{oi}-cut{k}", data[:(len(data) - 1) * (k + 1) // 17 + 1]
            for k in range(200):
                at, value = int(rng.integers(2, len(data))), int(rng.integers(0, 256))
                changed = bytearray(data)
                changed[at] = value
                yield f"{fmt}-o{oi}-byte{k}", bytes(changed)
