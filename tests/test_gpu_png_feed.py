"""PNG files decoded on the device: `yogo_png_unpack` (yogo_amd/csrc/png_unpack.hip) on hand-built scanlines of every filter type
and shape against the numpy restatement of the filters (tests/_png_write.py, held to PIL in tests/test_png_host.py);
`PngDeviceFeed` (yogo_amd/png_feed.py) on a directory of PIL-written files against `read_image`; `predict(...,
device_image_decode=True)` against the DataLoader route."""
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import _png_write as PW

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLASSES = ["you", "only", "glance", "once"]


def _unpack(scans, raws, H, W, crop=None, fp32=False, flags=None):
    """one launch over the images `scans` (uint8 [H, 1 + W] scanlines, or [H, W] pixels where raws[i]) -> (batch on the host, status)"""
    from yogo_amd.device_decode import center_crop_origin, png_unpack

    buf, table = bytearray(b"\xEE" * 16), []
    for s, raw in zip(scans, raws):
        buf += b"\xEE" * ((3 * len(table) + 1) % 7)        # images at every alignment
        table.append((len(buf), 1 if raw else 0))
        buf += np.ascontiguousarray(s, dtype=np.uint8).tobytes()
    OH, OW = crop or (H, W)
    top, left = center_crop_origin(H, W, OH, OW)
    out = torch.full((len(scans), 1, OH, OW), 7, dtype=torch.float32 if fp32 else torch.uint8, device="cuda")
    status = torch.full((len(scans),), -1, dtype=torch.int32, device="cuda")
    png_unpack(torch.frombuffer(buf, dtype=torch.uint8).cuda(), torch.tensor(table, dtype=torch.int64, device="cuda"), (H, W), out, status,
               top, left)
    return out.cpu(), status.cpu().tolist()


def _image(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(H, W), dtype=np.uint8)


@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("H", [1, 2, 65, 130])
def test_unpack_every_filter_and_shape(H, W):
    """one launch: every row one filter type (five images), a seeded random type per row, row 0 under types 2 / 3 / 4, and a
    raw-flagged image; uint8 and / 255"""
    rng = np.random.default_rng(H * 1000 + W)
    typesets = [[t] * H for t in range(5)] + [rng.integers(0, 5, size=H).tolist()] + [[t] + rng.integers(0, 5, size=H - 1).tolist() for t in (2, 3, 4)]
    imgs = [_image(H, W, 10 * i + H + W) for i in range(len(typesets) + 1)]
    scans = [PW.filter_rows(im, ts) for im, ts in zip(imgs, typesets)] + [imgs[-1]]
    for s, ts, im in zip(scans, typesets, imgs):
        assert s[:, 0].tolist() == ts and np.array_equal(PW.unfilter_rows(s), im)
    raws = [False] * len(typesets) + [True]
    want = torch.from_numpy(np.stack(imgs))[:, None]
    got, status = _unpack(scans, raws, H, W)
    assert status == [0] * len(imgs) and torch.equal(got, want)
    got, status = _unpack(scans, raws, H, W, fp32=True)
    assert status == [0] * len(imgs) and torch.equal(got, want / 255)


@pytest.mark.parametrize("H,W,crop", [(130, 65, (64, 65)), (65, 130, (33, 100)), (24, 48, (12, 48)), (5, 7, (1, 1))])
def test_unpack_centre_crop(H, W, crop):
    from yogo_amd.image_path_dataset import CenterCrop

    imgs = [_image(H, W, s) for s in range(3)]
    scans = [PW.filter_rows(imgs[0], [4] * H), PW.filter_rows(imgs[1], [(y * 3) % 5 for y in range(H)]), imgs[2]]
    want = CenterCrop(crop)(torch.from_numpy(np.stack(imgs))[:, None])
    got, status = _unpack(scans, [False, False, True], H, W, crop=crop)
    assert status == [0, 0, 0] and torch.equal(got, want)
    got, _ = _unpack(scans, [False, False, True], H, W, crop=crop, fp32=True)
    assert torch.equal(got, want / 255)


def test_unpack_bad_filter_byte_and_bad_image():
    from yogo_amd.device_decode import png_unpack

    H, W = 70, 20
    imgs = [_image(H, W, s) for s in range(3)]
    scans = [PW.filter_rows(im, [1] * H) for im in imgs]
    scans[1][66, 0] = 5             # in the second band of 64 rows
    got, status = _unpack(scans, [False] * 3, H, W)
    assert status == [0, 1, 0]
    assert torch.equal(got[0, 0], torch.from_numpy(imgs[0])) and torch.equal(got[2, 0], torch.from_numpy(imgs[2]))
    assert torch.equal(got[1, 0, :64], torch.from_numpy(imgs[1][:64]))          # the band before the bad byte is whole
    # images that do not lie inside the buffer are refused before anything of them is read
    scan = torch.zeros(H * (W + 1) + 8, dtype=torch.uint8, device="cuda")
    table = torch.tensor([(-1, 0), (9, 0), (1 << 62, 0), (8, 0), (H * (W + 1) + 8 - H * W + 1, 1)], dtype=torch.int64, device="cuda")
    out = torch.zeros((5, 1, H, W), dtype=torch.uint8, device="cuda")
    status = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    png_unpack(scan, table, (H, W), out, status)
    assert status.cpu().tolist() == [2, 2, 2, 0, 2]


@pytest.fixture(scope="module")
def png_dir(tmp_path_factory):
    """ten 24 x 48 grey files written by PIL (smooth plus noise: PIL picks several filter types), one RGB, one 16-bit and one
    interlaced file, and the frames `read_image` gives for all of them"""
    from yogo_amd.yogo_dataset import read_image

    d = tmp_path_factory.mktemp("pngs")
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:24, 0:48]
    for i in range(10):
        Image.fromarray(((yy * (i + 1) + xx * 3) + rng.integers(0, 20, size=(24, 48))).astype(np.uint8)).save(d / f"img_{i:02d}.png")
    Image.fromarray(rng.integers(0, 256, size=(24, 48, 3), dtype=np.uint8)).save(d / "img_10_rgb.png")
    Image.fromarray(rng.integers(0, 65536, size=(24, 48), dtype=np.uint16)).save(d / "img_11_16bit.png")
    lace = _image(24, 48, 5)      # (PIL writes no interlaced files: this one is built by hand; PIL reads it)
    (d / "img_12_interlaced.png").write_bytes(PW.png_bytes(lace, ihdr=(48, 24, 8, 0, 0, 0, 1), scan=PW.adam7_scan(lace)))
    assert torch.equal(read_image(d / "img_12_interlaced.png")[0], torch.from_numpy(lace))
    paths = sorted(str(p) for p in d.glob("*.png"))
    return d, paths, torch.stack([read_image(p) for p in paths])


def _feed(d, batch, **kw):
    from yogo_amd.image_path_dataset import ImagePathDataset
    from yogo_amd.png_feed import PngDeviceFeed

    return PngDeviceFeed(ImagePathDataset(d), batch, "cuda", **kw)


@pytest.mark.parametrize("batch", [4, 13, 5])
def test_feed_batches_equal_read_image(png_dir, batch):
    from yogo_amd import _hip

    d, paths, want = png_dir
    _hip.launch_log(True)
    try:
        feed = _feed(d, batch)
        batches = list(feed)
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    assert [b.shape[0] for b, _ in batches] == [min(batch, 13 - lo) for lo in range(0, 13, batch)]      # a partial last batch
    assert all(b.is_cuda and b.dtype == torch.uint8 for b, _ in batches)
    assert [n for _, names in batches for n in names] == paths
    assert torch.equal(torch.cat([b.cpu() for b, _ in batches]), want)
    assert feed.host_decoded == 3
    inflates = sum(ln.startswith("inflate_zlib_kernel") for ln in log)
    assert inflates == sum(1 for lo in range(0, 13, batch) if lo < 10) and sum(ln.startswith("png_unpack_kernel") for ln in log) == len(batches)
    f32 = torch.cat([b.cpu() for b, _ in _feed(d, batch, normalize=True, crop=(12, 48))])
    assert f32.dtype == torch.float32 and torch.equal(f32, want[:, :, 6:18] / 255)


@pytest.mark.parametrize("defect", ["flipped-idat-byte", "other-size", "bad-filter-byte", "short-scanlines", "stale-crc-fixed"])
def test_feed_bad_file_costs_exactly_its_batch(png_dir, tmp_path, defect):
    import shutil
    import zlib

    d, paths, want = png_dir
    for p in paths[:10]:
        shutil.copy(p, tmp_path)
    victim = tmp_path / "img_05.png"
    data = victim.read_bytes()
    img = want[5, 0].numpy()
    if defect == "flipped-idat-byte":          # the chunk's CRC-32 no longer fits
        at = data.index(b"IDAT") + 30
        data = data[:at] + bytes([data[at] ^ 0x40]) + data[at + 1:]
    elif defect == "stale-crc-fixed":          # the same flip with the CRC-32 made good: the device's checks are left to find it
        at = data.index(b"IDAT")
        n = int.from_bytes(data[at - 4:at], "big")
        body = bytearray(data[at:at + 4 + n])
        body[30] ^= 0x40
        data = data[:at] + bytes(body) + zlib.crc32(bytes(body)).to_bytes(4, "big") + data[at + 8 + n:]
    elif defect == "other-size":
        data = PW.png_bytes(_image(24, 40, 1))
    elif defect == "bad-filter-byte":
        scan = PW.filter_rows(img, [0] * 24)
        scan[7, 0] = 9
        data = PW.png_bytes(img, scan=scan.tobytes())
    else:                                      # a stream that inflates to one row less than the header announces
        data = PW.png_bytes(img, scan=PW.filter_rows(img, [1] * 24).tobytes()[:-49])
    victim.write_bytes(data)
    feed = _feed(tmp_path, 4)
    b0, n0 = next(feed)
    assert torch.equal(b0.cpu(), want[:4])
    with pytest.raises(RuntimeError, match="img_05"):
        next(feed)
    b2, n2 = next(feed)
    assert torch.equal(b2.cpu(), want[8:10]) and [Path(n).name for n in n2] == ["img_08.png", "img_09.png"]
    with pytest.raises(StopIteration):
        next(feed)


def test_feed_file_larger_than_the_room_and_not_a_png(png_dir, tmp_path):
    """a file whose stream is longer than the room sized from the first batch, and a JPEG under a .png name, go through the host"""
    import shutil

    from yogo_amd.yogo_dataset import read_image

    d, paths, want = png_dir
    for p in paths[:6]:
        shutil.copy(p, tmp_path)
    import zlib

    from yogo_amd import png

    noise = _image(24, 48, 77)
    c = zlib.compressobj(1)       # a sync flush after every byte: six bytes of stream per byte of scanline
    scan = PW.filter_rows(noise, [0] * 24).tobytes()
    stream = b"".join(c.compress(scan[i:i + 1]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(len(scan))) + c.flush()
    (tmp_path / "img_04.png").write_bytes(PW.png_bytes(noise, stream=stream, idat_sizes=[100] * 8))
    assert png.parse_png((tmp_path / "img_04.png").read_bytes()).device_decodable
    Image.fromarray(want[5, 0].numpy()).save(tmp_path / "img_05.png", format="BMP")
    feed = _feed(tmp_path, 2)
    got = torch.cat([b.cpu() for b, _ in feed])
    assert 0 < feed.room < len(stream)
    assert torch.equal(got[:4], want[:4]) and torch.equal(got[4, 0], torch.from_numpy(noise))
    assert torch.equal(got[5], read_image(tmp_path / "img_05.png")) and feed.host_decoded == 2


def _make_checkpoint(tmp_path, seed=3, is_rgb=False):
    """as tests/test_gpu_cli.py::_make_checkpoint"""
    from yogo_amd.model import YOGO

    torch.manual_seed(seed)
    net = YOGO((64, 96), 0.0425, 0.0555, 4, is_rgb=is_rgb).cuda()
    net.eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 50.0)
                m.running_var.uniform_(2000.0, 9000.0)
        net.model[7].bias[4] += 1.5
    p = tmp_path / "m.pth"
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "fake_model",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, p)
    return p


@pytest.mark.parametrize("crop", [None, 0.5])
def test_predict_with_device_image_decode_equals_predict_without(tmp_path, capsys, crop):
    from yogo_amd import _hip
    from yogo_amd.infer import predict

    pth = _make_checkpoint(tmp_path)
    imgdir = ROOT / "tests/fake-data/data/images1"
    kw = dict(save_npy=True, count_predictions=True, batch_size=2, obj_thresh=0.4, iou_thresh=0.5, class_names=CLASSES, vertical_crop_height=crop)
    predict(str(pth), path_to_images=imgdir, output_dir=str(tmp_path / "host"), **kw)
    host_out = capsys.readouterr().out
    _hip.launch_log(True)
    try:
        predict(str(pth), path_to_images=imgdir, output_dir=str(tmp_path / "dev"), device_image_decode=True, **kw)
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    assert capsys.readouterr().out == host_out and "you" in host_out
    a, b = sorted((tmp_path / "host").glob("*.npy")), sorted((tmp_path / "dev").glob("*.npy"))
    assert len(a) == 1 and [p.name for p in a] == [p.name for p in b] and a[0].read_bytes() == b[0].read_bytes()
    assert np.load(a[0]).shape[1] > 0
    assert any(ln.startswith("png_unpack_kernel") for ln in log)
    with pytest.raises(ValueError, match="zarr"):
        predict(str(pth), path_to_zarr=tmp_path / "x.zarr", device_image_decode=True)


def test_flag_is_refused_for_an_rgb_model(tmp_path):
    from yogo_amd.infer import predict

    pth = _make_checkpoint(tmp_path, is_rgb=True)
    with pytest.raises(ValueError, match="RGB"):
        predict(str(pth), path_to_images=ROOT / "tests/fake-data/data/images1", device_image_decode=True)


def test_infer_flag_parses():
    from yogo_amd.utils.argparsers import global_parser

    args = global_parser().parse_args(["infer", "m.pth", "--path-to-images", "imgs", "--device-image-decode"])
    assert args.device_image_decode is True
    assert global_parser().parse_args(["infer", "m.pth", "--path-to-images", "imgs"]).device_image_decode is False
