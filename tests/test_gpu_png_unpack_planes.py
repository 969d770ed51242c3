"""`yogo_png_unpack_planes` (csrc/png_unpack_planes.hip) on the MI355X: scanlines of 8-bit greyscale and RGB files -> 1 or 3
planes, bit for bit what ``read_image(file, rgb)`` gives of the same file, bit for bit ``yogo_png_unpack`` where the two overlap,
and the two checks the kernel makes itself (a filter-type byte above 4, an image outside the scanline buffer).

Shapes: H in {1, 64, 65, 129} -- one band, the band edge, three bands; W in {1, 2, 5, 67} -- a lone pixel, a four-pixel fetch
that crosses the row end, W > 64 so that the row above is reloaded in the middle of a row."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from _png_write import filter_rows, png_bytes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HS, WS = (1, 64, 65, 129), (1, 2, 5, 67)
ALIGN = 16


@lru_cache(maxsize=None)
def _images(H, W):
    """the images of one launch, seeded: [(name, pixels [H, W] or [H, W, 3], filter type per row)]"""
    rng = np.random.default_rng(H * 1000 + W)
    out = []
    for rgb in (False, True):
        shape = (H, W, 3) if rgb else (H, W)
        tag = "rgb" if rgb else "grey"
        for t in range(5):
            out.append((f"{tag}_f{t}", rng.integers(0, 256, size=shape, dtype=np.uint8), (t,) * H))
        out.append((f"{tag}_mixed", rng.integers(0, 256, size=shape, dtype=np.uint8), tuple(int(t) for t in rng.integers(0, 5, size=H))))
        # pixels from {0, 1, 255}: Paeth ties and Average carries
        out.append((f"{tag}_ties", rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=shape), tuple(int(t) for t in rng.integers(3, 5, size=H))))
    return out


def _pack(blobs):
    """byte strings -> (one uint8 array with every blob at a multiple of ALIGN, their offsets)"""
    offs, at = [], 0
    for b in blobs:
        offs.append(at)
        at += -(-len(b) // ALIGN) * ALIGN
    buf = np.zeros(max(at, 1), dtype=np.uint8)
    for o, b in zip(offs, blobs):
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return buf, offs


def _launch(scan_np, table, hw, C, B, fill=0xA5):
    from yogo_amd.device_decode import png_unpack_planes

    scan = torch.from_numpy(scan_np.copy()).to(DEV)   # (the kernel writes into the scanlines: every launch has its own)
    out = torch.full((B, C, *hw), fill, dtype=torch.uint8, device=DEV)
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    png_unpack_planes(scan, torch.tensor(table, dtype=torch.int64, device=DEV), hw, out, status)
    torch.cuda.synchronize()
    return out.cpu(), status.cpu()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("H", HS)
def test_planes_equal_read_image(tmp_path, H, W, C):
    from yogo_amd.device_decode import png_unpack
    from yogo_amd.yogo_dataset import read_image

    images = _images(H, W)
    want, blobs, kinds = [], [], []
    for name, px, types in images:
        p = tmp_path / f"{name}.png"
        p.write_bytes(png_bytes(px, types))
        want.append(read_image(p, rgb=C == 3))
        blobs.append(filter_rows(px, types).tobytes())
        kinds.append(2 if px.ndim == 3 else 0)
    planar = np.random.default_rng(7).integers(0, 256, size=(C, H, W), dtype=np.uint8)   # an image the host decoded
    want.append(torch.from_numpy(planar))
    blobs.append(planar.tobytes())
    kinds.append(1)
    scan, offs = _pack(blobs)
    B = len(blobs)
    out, status = _launch(scan, list(zip(offs, kinds)), (H, W), C, B)
    assert status.tolist() == [0] * B
    for b in range(B):
        assert torch.equal(out[b], want[b]), (images[b][0] if b < len(images) else "planar", H, W, C)
    if C == 1:   # the grey images again through yogo_png_unpack: the same bytes
        grey = [b for b, k in enumerate(kinds) if k == 0]
        old = torch.zeros((len(grey), 1, H, W), dtype=torch.uint8, device=DEV)
        st = torch.full((len(grey),), -1, dtype=torch.int32, device=DEV)
        png_unpack(torch.from_numpy(scan.copy()).to(DEV), torch.tensor([(offs[b], 0) for b in grey], dtype=torch.int64, device=DEV), (H, W), old, st)
        assert st.tolist() == [0] * len(grey) and torch.equal(old.cpu(), out[grey])


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("bad", ["grey", "rgb"])
def test_filter_byte_above_4_is_that_images_status(bad, C):
    H, W = 129, 5
    rng = np.random.default_rng(3)
    grey = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    types = [int(t) for t in rng.integers(0, 5, size=H)]
    blobs = [filter_rows(grey, types), filter_rows(rgb, types), filter_rows(grey, types), filter_rows(rgb, types)]
    victim = 2 if bad == "grey" else 1
    blobs[victim] = blobs[victim].copy()
    blobs[victim][70, 0] = 5   # in the second band: the first band's rows are still written
    scan, offs = _pack([b.tobytes() for b in blobs])
    out, status = _launch(scan, list(zip(offs, [0, 2, 0, 2])), (H, W), C, 4)
    assert status.tolist() == [1 if b == victim else 0 for b in range(4)]
    g = torch.from_numpy(grey)[None]
    r = torch.from_numpy(rgb).permute(2, 0, 1)
    lum = ((19595 * r[0].int() + 38470 * r[1].int() + 7471 * r[2].int() + 0x8000) >> 16).to(torch.uint8)[None]
    want = [g.expand(C, H, W), r if C == 3 else lum, g.expand(C, H, W), r if C == 3 else lum]
    for b in range(4):
        if b != victim:
            assert torch.equal(out[b], want[b]), b
    assert torch.equal(out[victim][:, :64], want[victim][:, :64]) and bool((out[victim][:, 64:] == 0xA5).all())


@pytest.mark.parametrize("C", [1, 3])
def test_an_image_outside_the_scanlines_is_status_2(C):
    H, W = 65, 5
    rng = np.random.default_rng(5)
    grey = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    types = [int(t) for t in rng.integers(0, 5, size=H)]
    scan, offs = _pack([filter_rows(grey, types).tobytes(), filter_rows(rgb, types).tobytes()])
    n = len(scan)
    # past the end, ending one byte after the end (an RGB image at the grey one's distance from the end), negative, an unknown kind
    table = [(offs[0], 0), (n + 4096, 0), (offs[1], 2), (n - H * (W + 1), 2), (-16, 1), (offs[0], 3), (n - H * (W + 1) + 1, 0)]
    out, status = _launch(scan, table, (H, W), C, len(table))
    assert status.tolist() == [0, 2, 0, 2, 2, 2, 2]
    g = torch.from_numpy(grey)[None].expand(C, H, W)
    r = torch.from_numpy(rgb).permute(2, 0, 1)
    lum = ((19595 * r[0].int() + 38470 * r[1].int() + 7471 * r[2].int() + 0x8000) >> 16).to(torch.uint8)[None]
    assert torch.equal(out[0], g) and torch.equal(out[2], r if C == 3 else lum)
    for b in (1, 3, 4, 5, 6):
        assert bool((out[b] == 0xA5).all()), b


def test_rgb_to_one_plane_is_pils_luma(tmp_path):
    """every (R, G, B) of a 65 x 65 x 65 lattice (0, 4, ..., 252, 255 per channel) through the kernel == PIL's convert('L')"""
    from yogo_amd.yogo_dataset import read_image

    v = np.concatenate((np.arange(0, 256, 4), [255])).astype(np.uint8)
    lattice = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)
    H, W = 65, 65 * 65
    img = lattice.reshape(H, W, 3)
    p = tmp_path / "lattice.png"
    p.write_bytes(png_bytes(img))
    scan, offs = _pack([filter_rows(img, [0] * H).tobytes()])
    out, status = _launch(scan, [(offs[0], 2)], (H, W), 1, 1)
    assert status.tolist() == [0] and torch.equal(out[0], read_image(p, rgb=False))
