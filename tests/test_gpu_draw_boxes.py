"""`yogo infer --draw-boxes --device-draw` on the device: the render kernel against its numpy twin (tests/_draw_ref.py, itself held to
PIL in tests/test_draw_host.py), the PNG encoder against its pure-Python twin byte for byte and through the repository's own device
decoders, a slot that is too small, and ``predict`` end to end against the host route: same file names, same pixels."""
import ctypes

import numpy as np
import pytest
import torch

import _draw_ref as R
import _zarr_write as ZW
from yogo_amd import draw
from yogo_amd import png_encode as E

pytestmark = pytest.mark.gpu
C = len(R.CLASS_NAMES)
CLASSES = ["you", "only", "glance", "once"]


@pytest.fixture(scope="module")
def atlas():
    return draw.GlyphAtlas(R.CLASS_NAMES)


def _batch(cases, cap):
    """cases [(img, rows)] -> (images [B, ch, H, W], rows [B, cap, 5 + C] padded with junk, counts [B])"""
    B = len(cases)
    rows = np.random.default_rng(1).uniform(0, 1, (B, cap, 5 + C)).astype(np.float32)   # rows past the count must not be drawn
    counts = np.zeros(B, dtype=np.int32)
    for b, (_, r) in enumerate(cases):
        rows[b, : len(r)] = r
        counts[b] = len(r)
    return np.stack([img for img, _ in cases]), rows, counts


def _render_and_compare(atlas, cases, cap, as_float):
    imgs, rows, counts = _batch(cases, cap)
    channels = imgs.shape[1]
    dev = draw.DeviceAtlas(atlas, channels, "cuda")
    x = torch.from_numpy(imgs).cuda()
    if as_float:
        x = x / 255      # what a normalising loader hands the model (fp32)
    got = draw.render_boxes(x, torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(), dev, normalised=as_float).cpu().numpy()
    colours = draw.colour_table(C, channels)
    for b, (img, r) in enumerate(cases):
        src = x[b].cpu().numpy() if as_float else img
        want = R.render(src, r, atlas, colours, normalised=as_float)
        assert np.array_equal(got[b], want), f"image {b}: {int((got[b] != want).any(-1).sum())} pixels differ"


@pytest.mark.parametrize("as_float", [False, True], ids=["uint8", "normalised"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("hw", [(48, 64), (53, 71)])
def test_render_equals_twin(atlas, hw, channels, as_float):
    cap = 8
    cases = R.make_cases(seed=hw[0] * channels, n_cases=24, H=hw[0], W=hw[1], channels=channels, max_boxes=cap)
    rng = np.random.default_rng(9)
    cases[1] = (cases[1][0], R.random_rows(rng, cap, C))      # counts == cap beside case 0's counts == 0
    assert len(cases[0][1]) == 0 and len(cases[1][1]) == cap
    for k in range(0, len(cases), 3):
        _render_and_compare(atlas, cases[k: k + 3], cap, as_float)


def test_render_more_rows_than_one_pass_takes(atlas):
    """the kernel takes an image's rows 256 at a time: 300 and 257 rows cross that, in order"""
    rng = np.random.default_rng(4)
    imgs = rng.integers(0, 256, (3, 1, 48, 64), dtype=np.uint8)
    cases = [(imgs[0], R.random_rows(rng, 300, C)), (imgs[1], R.random_rows(rng, 257, C)), (imgs[2], R.random_rows(rng, 0, C))]
    _render_and_compare(atlas, cases, 300, False)


def test_render_refuses_bad_arguments(atlas):
    dev = draw.DeviceAtlas(atlas, 1, "cuda")
    x = torch.zeros(3, 1, 48, 64, dtype=torch.uint8, device="cuda")
    rows, counts = torch.zeros(3, 8, 5 + C, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        draw.render_boxes(x[:, :, :, :, None], rows, counts, dev, False)
    with pytest.raises(ValueError):
        draw.render_boxes(x, rows[:, :, :-1], counts, dev, False)
    with pytest.raises(RuntimeError):
        draw.render_boxes(x, rows.cpu(), counts, dev, False)


# ---- the encoder ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(atlas):
    img, rows = R.make_cases(seed=3, n_cases=4, H=48, W=64, channels=1)[2]
    return R.encoder_cases(R.render(img, rows, atlas, draw.colour_table(C, 1)))


def _files(files, offsets, status, slot=None):
    off = offsets.cpu().numpy()
    assert status.cpu().tolist() == [0] * (len(off) - 1)
    data = files.cpu().numpy()
    if slot is None:
        return [data[off[b]: off[b + 1]].tobytes() for b in range(len(off) - 1)]
    return [data[b * slot: b * slot + off[b + 1] - off[b]].tobytes() for b in range(len(off) - 1)]


@pytest.mark.parametrize("name", ["noise", "constant", "rendered", "one_pixel", "ragged_height", "wide_band", "few_values"])
def test_encoder_equals_twin(frames, name):
    px = frames[name]
    H, W, bpp = px.shape
    slot, _ = draw.encode_bound(H, W, bpp)
    assert slot == E.encode_bound(H, W, bpp)
    want = E.encode_png_host(px)
    got = _files(*draw.encode_png(torch.from_numpy(px[None]).cuda()), slot=slot)
    assert len(got[0]) == len(want) and got[0] == want


@pytest.mark.parametrize("packed", [False, True])
def test_encoder_batch_of_three(frames, packed):
    batch = np.stack([frames["noise"], frames["constant"], frames["rendered"]])
    slot, _ = draw.encode_bound(48, 64, 4)
    files, offsets, status = draw.encode_png(torch.from_numpy(batch).cuda(), packed=packed)
    got = _files(files, offsets, status, slot=None if packed else slot)
    assert got == [E.encode_png_host(px) for px in batch]


def test_encoder_other_pixel_sizes():
    rng = np.random.default_rng(8)
    for bpp in (1, 2, 3):
        px = (rng.integers(0, 5, (21, 33, bpp), dtype=np.uint8) * 50).astype(np.uint8)
        got = _files(*draw.encode_png(torch.from_numpy(px[None]).cuda(), packed=True))
        assert got[0] == E.encode_png_host(px)


def test_round_trip_through_the_device_decoders(frames):
    """the encoder's IDAT bytes through yogo_inflate_zlib and yogo_png_unpack_any (RGBA, 8 bits) give the planes the repository's
    host decoder gives for the same file"""
    from yogo_amd import device_decode as DD
    from yogo_amd import png
    from yogo_amd.inflate import split_zlib

    for name in ("rendered", "ragged_height", "noise"):
        px = frames[name]
        H, W, _ = px.shape
        files, offsets, status = draw.encode_png(torch.from_numpy(px[None]).cuda(), packed=True)
        assert int(status[0]) == 0
        data = files[: int(offsets[1])]
        host = data.cpu().numpy().tobytes()
        info = png.parse_png(host)
        assert (info.width, info.height, info.bit_depth, info.color_type, info.interlace) == (W, H, 8, 6, 0)
        stream = torch.cat([data[o: o + n] for o, n in info.idat])          # stays on the device
        off, length, adler = split_zlib(stream.cpu().numpy().tobytes())
        scan = torch.zeros((info.inflated_bytes + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        table = torch.tensor([[off, length, 0, info.inflated_bytes, adler]], dtype=torch.int64, device="cuda")
        st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        DD.inflate_streams(stream.contiguous(), table, scan, st)
        assert int(st[0]) == 0
        out = torch.zeros(1, 3, H, W, dtype=torch.uint8, device="cuda")
        st2 = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        DD.png_unpack_any(scan, torch.tensor([[0, info.format_code, 0]], dtype=torch.int64, device="cuda"), (H, W), out, st2)
        assert int(st2[0]) == 0
        want = png.decode_any(host, rgb=True)
        assert np.array_equal(out[0].cpu().numpy(), want) and np.array_equal(want, px[:, :, :3].transpose(2, 0, 1))


@pytest.mark.parametrize("packed", [False, True])
def test_slot_one_byte_too_small(frames, packed):
    """the noise frame needs the whole bound: one byte less is refused with a status and nothing is written, in or past the slot"""
    batch = np.stack([frames["constant"], frames["noise"]])
    slot, work_per = draw.encode_bound(48, 64, 4)
    small, guard = slot - 1, 4096
    files = torch.full((2 * small + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    _, offsets, status = draw.encode_png(torch.from_numpy(batch).cuda(), files=files, packed=packed, slot_bytes=small)
    want = E.encode_png_host(batch[0])
    assert status.cpu().tolist() == [0, E.ST_SLOT] and offsets.cpu().tolist() == [0, len(want), len(want)]
    host = files.cpu().numpy()
    assert host[: len(want)].tobytes() == want and (host[len(want):] == 0xA5).all()


def test_encoder_refuses_bad_arguments():
    from yogo_amd import _hip

    px = torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        draw.encode_png(px[:, :, :, :, None])
    with pytest.raises(ValueError):
        draw.encode_png(px, work=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    out = ctypes.c_size_t(0)
    with pytest.raises(RuntimeError):
        _hip.call("yogo_png_encode_bound", 0, 4, 4, ctypes.addressof(out), ctypes.addressof(out))
    with pytest.raises(RuntimeError):
        _hip.call("yogo_png_encode_bound", 4, 4, 5, ctypes.addressof(out), ctypes.addressof(out))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _make_checkpoint(tmp_path, seed=3, normalize=False):
    """as tests/test_gpu_cli.py::_make_checkpoint: random-init base_model whose statistics let a handful of cells fire"""
    from yogo_amd.model import YOGO

    torch.manual_seed(seed)
    net = YOGO((64, 96), 0.0425, 0.0555, 4).cuda()
    net.eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 50.0)
                m.running_var.uniform_(2000.0, 9000.0)
        net.model[7].bias[4] += 1.5
    p = tmp_path / "m.pth"
    torch.save({"epoch": 0, "step": 7, "normalize_images": normalize, "classes": CLASSES, "model_name": "fake_model",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, p)
    return p


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """ten random 64 x 96 frames as a PNG directory and as a zarr zip, and a checkpoint"""
    from PIL import Image

    d = tmp_path_factory.mktemp("draw_e2e")
    frames = np.random.default_rng(6).integers(0, 256, size=(64, 96, 10), dtype=np.uint8)
    (d / "png").mkdir()
    for i in range(10):
        Image.fromarray(frames[:, :, i]).save(d / "png" / f"img_{i:02d}.png")
    z = ZW.write_stack(d / "stack.zip", frames, (64, 96, 1), as_zip=True)
    return d / "png", z, _make_checkpoint(d)


def _same_pixels(a, b, suffix, n):
    from PIL import Image

    fa, fb = sorted(p.name for p in a.iterdir()), sorted(p.name for p in b.iterdir())
    assert fa == fb and len(fa) == n and all(f.endswith(suffix) for f in fa)
    drawn = 0
    for f in fa:
        ia, ib = Image.open(a / f), Image.open(b / f)
        assert ia.mode == ib.mode == "RGBA" and ia.size == ib.size == (96, 64)
        pa, pb = np.asarray(ia), np.asarray(ib)
        assert np.array_equal(pa, pb), f"{f}: {int((pa != pb).any(-1).sum())} pixels differ"
        drawn += int((pa[:, :, 0] != pa[:, :, 1]).any() or (pa[:, :, 1] != pa[:, :, 2]).any())   # a coloured outline on a grey image
    assert drawn > 0, "no image has a box: the comparison shows nothing"


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("source,suffix", [("png", ".png"), ("zarr", ".png"), ("png", ".tif")])
def test_predict_device_draw_writes_the_same_pixels(e2e, tmp_path, half, source, suffix):
    from yogo_amd.infer import predict

    pngs, z, pth = e2e
    src = dict(path_to_images=pngs) if source == "png" else dict(path_to_zarr=z)
    kw = dict(draw_boxes=True, batch_size=4, obj_thresh=0.4, iou_thresh=0.5, half=half, class_names=CLASSES, output_img_ftype=suffix, **src)
    predict(str(pth), output_dir=str(tmp_path / "a"), **kw)
    predict(str(pth), output_dir=str(tmp_path / "b"), device_draw=True, **kw)
    _same_pixels(tmp_path / "a", tmp_path / "b", suffix, 10)


def test_predict_device_draw_fake_data_images(tmp_path):
    """the fake-data PNG directory of tests/test_gpu_cli.py, default labels (class numbers)"""
    from pathlib import Path

    from yogo_amd.infer import predict

    imgdir = Path(__file__).resolve().parent / "fake-data" / "data" / "images1"
    pth = _make_checkpoint(tmp_path, normalize=False)
    kw = dict(path_to_images=imgdir, draw_boxes=True, batch_size=2, obj_thresh=0.4)
    predict(str(pth), output_dir=str(tmp_path / "a"), **kw)
    predict(str(pth), output_dir=str(tmp_path / "b"), device_draw=True, **kw)
    _same_pixels(tmp_path / "a", tmp_path / "b", ".png", 3)
