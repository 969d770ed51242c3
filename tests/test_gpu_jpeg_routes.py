"""The routes behind ``--device-image-decode-jpeg`` on the MI355X against the host routes: the prefill of the device image cache,
the labelled stream, the prefill's resize and the inference feed.

The data set: ten images at 35 x 37 with label files of 0, 1 and several lines -- two grey ``.jpg``, a 4:2:0 ``.jpg``, a ``.jpg``
with restart markers, two ``.png`` files, a JPEG under a ``.png`` name, a progressive ``.jpg`` (the host's), a truncated ``.jpg``
(the kernel hands it back; PIL cannot read it either: unreadable on every route) and one grey ``.jpg`` at 70 x 74."""
import io
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import _jpeg_files as F

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:could not read")]
DEV = torch.device("cuda", 0)
HW = (35, 37)
Sx, Sy = 12, 8
N = 10
CLASSES = ["you", "only", "glance", "once"]
PNGS, PROGRESSIVE, TRUNCATED, BIG = (4, 5), 7, 8, 9
JPEGS = N - len(PNGS)


def _png(a: np.ndarray) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(a, "L").save(buf, format="PNG")
    return buf.getvalue()


def _files(rng):
    """name -> bytes of the ten files"""
    H, W = HW
    whole = F.write("grey", H, W, 90, "ramp", rng)
    buf = io.BytesIO()
    Image.fromarray(F.content("ramp", H, W, 1, rng)[..., 0], "L").save(buf, format="JPEG", progressive=True)
    return {
        "img_0000.jpg": F.write("grey", H, W, 90, "noise", rng),
        "img_0001.jpg": F.write("grey", H, W, 75, "ramp", rng, optimize=True),
        "img_0002.jpg": F.write("420", H, W, 85, "ramp", rng),
        "img_0003.jpg": F.write("422", H, W, 85, "noise", rng, restart_marker_blocks=3),
        "img_0004.png": _png(F.content("noise", H, W, 1, rng)[..., 0]),
        "img_0005.png": _png(F.content("ramp", H, W, 1, rng)[..., 0]),
        "img_0006.png": F.write("444", H, W, 95, "ramp", rng),
        "img_0007.jpg": buf.getvalue(),
        "img_0008.jpg": whole[:len(whole) // 2],
        "img_0009.jpg": F.write("grey", 2 * H, 2 * W, 90, "ramp", rng),
    }


def _dataset(root: Path, replace=None):
    img_dir, lab_dir = root / "images", root / "labels"
    img_dir.mkdir(parents=True)
    lab_dir.mkdir(parents=True)
    rng = np.random.default_rng(5)
    files = _files(rng)
    for name, data in files.items():
        if replace and name in replace:
            name, data = replace[name](data)
        (img_dir / name).write_bytes(data)
    for k in range(N):
        m = (0, 1, 4, 2, 0, 3, 1, 5, 2, 1)[k]
        lines = [f"{int(rng.integers(0, len(CLASSES)))} {rng.uniform(0.05, 0.95):.6f} {rng.uniform(0.05, 0.95):.6f} "
                 f"{rng.uniform(0.05, 0.3):.6f} {rng.uniform(0.05, 0.3):.6f}" for _ in range(m)]
        (lab_dir / f"img_{k:04d}.txt").write_text("".join(ln + "\n" for ln in lines))
    return img_dir, lab_dir


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from yogo_amd.dataset_definition_file import DatasetDefinition

    root = tmp_path_factory.mktemp("jpeg_routes")
    img_dir, lab_dir = _dataset(root / "data")
    yml = root / "defn.yml"
    yml.write_text("class_names: [you, only, glance, once]\ndataset_split_fractions: {train: 0.7, val: 0.3}\n"
                   f"dataset_paths:\n  a: {{image_path: {img_dir}, label_path: {lab_dir}}}\n")
    return root, img_dir, lab_dir, DatasetDefinition.from_yaml(yml)


def _split(img_dir, lab_dir, rgb=False):
    from yogo_amd.yogo_dataset import ObjectDetectionDataset

    split = ObjectDetectionDataset(img_dir, lab_dir, Sx, Sy, CLASSES, image_hw=HW, rgb=rgb)
    assert len(split) == N and [Path(str(p)).stem for p in split._image_paths] == [f"img_{k:04d}" for k in range(N)]
    return split


def _cache(split, rgb=False, **kw):
    from yogo_amd.image_cache import ImageCache

    c = ImageCache(split, N, (3 if rgb else 1, *HW), False, device=DEV, num_workers=0, batch_size=4, decode_batch=4, **kw)
    c.images.fill_(0x5A)
    c.prefill()
    return c


_HOST = {}


def _host_cache(data, rgb):
    if rgb not in _HOST:
        _HOST[rgb] = _cache(_split(*data[1:3], rgb=rgb), rgb)
    return _HOST[rgb]


@pytest.mark.parametrize("rgb", [False, True])
def test_prefill_with_the_switch_equals_the_host_route(data, rgb):
    from yogo_amd import _hip

    host = _host_cache(data, rgb)
    _hip.launch_log(True)
    try:
        dev = _cache(_split(*data[1:3], rgb=rgb), rgb, device_decode=True, device_decode_jpeg=True)
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    assert host.resident.tolist() == [k != TRUNCATED for k in range(N)] and np.array_equal(dev.resident, host.resident)
    # (the truncated file's slot is not resident on either route; here it holds what the kernel decoded before the source ended,
    # as the slot of a PNG whose inflate fails does)
    keep = np.flatnonzero(host.resident).tolist()
    assert torch.equal(dev.images[keep].cpu(), host.images[keep].cpu())
    assert torch.equal(dev.rows, host.rows) and np.array_equal(dev.row_offsets, host.row_offsets)
    assert {0, 2, 4} <= set(np.diff(dev.row_offsets).tolist())   # (a one-line label file reads as no row: its line is taken for a header)
    st = dev.decode_stats
    assert st["host_decoded"] == 3 and st["jpeg_decoded"] == JPEGS - 3      # the progressive, the truncated and the 70 x 74 file
    assert len(st["jpeg_ms"]) == 3 and all(t > 0 for t in st["jpeg_ms"])    # chunks of 4, 4 and 2: each has JPEG files
    assert sum(ln.startswith("jpeg_decode_kernel") for ln in log) == 3


def test_prefill_without_the_switch_is_unchanged(data):
    from yogo_amd import _hip

    host = _host_cache(data, False)
    _hip.launch_log(True)
    try:
        dev = _cache(_split(*data[1:3]), device_decode=True)
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    assert torch.equal(dev.images.cpu(), host.images.cpu()) and np.array_equal(dev.resident, host.resident)
    assert dev.decode_stats["host_decoded"] == JPEGS and "jpeg_decoded" not in dev.decode_stats and "jpeg_ms" not in dev.decode_stats
    assert len(dev.decode_stats["inflate_ms"]) == 1 and len(dev.decode_stats["unpack_ms"]) == 3
    assert not any(ln.startswith("jpeg_decode_kernel") for ln in log)


def _run(dls):
    out = {}
    for name in ("train", "val"):
        dls[name].sampler.set_epoch(0)
        torch.manual_seed(100)
        out[name] = [(i.cpu(), l.cpu()) for i, l in dls[name]]
    return out


def _loaders(data, **kw):
    from yogo_amd.yogo_dataloader import get_dataloader

    return get_dataloader(data[3], 4, Sx, Sy, image_hw=HW, device=DEV, training=True, **kw)


def _assert_same(got, want):
    for name in ("train", "val"):
        assert len(got[name]) == len(want[name]) > 0
        for k, ((gi, gl), (wi, wl)) in enumerate(zip(got[name], want[name])):
            assert gi.dtype == wi.dtype and gi.shape == wi.shape and torch.equal(gi, wi), (name, k)
            assert gl.dtype == wl.dtype and gl.shape == wl.shape and torch.equal(gl, wl), (name, k)


@pytest.mark.parametrize("rgb", [False, True])
def test_stream_with_the_switch_equals_the_worker_route(data, rgb):
    want = _run(_loaders(data, rgb=rgb))
    dls = _loaders(data, rgb=rgb, device_image_stream=True, device_image_decode_jpeg=True, stream_decode_batch=5)
    got = _run(dls)
    _assert_same(got, want)
    assert got["train"][0][0].dtype == torch.uint8 and got["train"][0][0].shape[1] == (3 if rgb else 1)
    stats = [dls[name].stream.stats for name in ("train", "val")]
    assert sum(s["streamed"] for s in stats) == N and sum(s["host_decoded"] for s in stats) == 3
    assert sum(s["jpeg_decoded"] for s in stats) == JPEGS - 3 and sum(len(s["jpeg_ms"]) for s in stats) >= 2
    dls["train"].stream.scratch.close()


def test_cached_batches_with_the_switch_equal_the_host_prefills(data):
    want = _run(_loaders(data, device_image_cache_gib=0.01))
    dls = _loaders(data, device_image_cache_gib=0.01, device_image_decode=True, device_image_decode_jpeg=True)
    _assert_same(_run(dls), want)
    assert sum(dls[name].cache.decode_stats["jpeg_decoded"] for name in ("train", "val")) == JPEGS - 3


def test_resized_jpeg_equals_a_png_of_the_same_pixels(data, tmp_path):
    """with device_resize the 70 x 74 JPEG stays on the device; its slot is, bit for bit, the slot a PNG holding the same decoded
    pixels gets through the device's resize route"""
    def as_png(jpeg_bytes):
        return "img_0009.png", _png(F.pil_pixels(jpeg_bytes, False)[0])

    img_dir, lab_dir = _dataset(tmp_path / "as_png", {"img_0009.jpg": as_png})
    want = _cache(_split(img_dir, lab_dir), device_decode=True, device_resize=True)
    assert want.decode_stats["device_resized"] == 1
    dev = _cache(_split(*data[1:3]), device_decode=True, device_resize=True, device_decode_jpeg=True)
    assert dev.decode_stats["device_resized"] == 1 and dev.decode_stats["host_decoded"] == 2 and dev.decode_stats["jpeg_decoded"] == JPEGS - 2
    assert dev.resident[BIG] and torch.equal(dev.images[BIG].cpu(), want.images[BIG].cpu())
    keep = [k for k in range(N) if k not in (BIG, TRUNCATED)]
    assert torch.equal(dev.images[keep].cpu(), _host_cache(data, False).images[keep].cpu())


def test_predict_takes_a_jpeg_under_a_png_name(tmp_path, capsys):
    from yogo_amd import _hip
    from yogo_amd.infer import predict
    from yogo_amd.model import YOGO

    torch.manual_seed(3)
    net = YOGO((64, 96), 0.0425, 0.0555, 4).cuda()
    net.eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 50.0)
                m.running_var.uniform_(2000.0, 9000.0)
        net.model[7].bias[4] += 1.5
    pth = tmp_path / "m.pth"
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "fake_model",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, pth)
    imgdir = tmp_path / "run" / "images"
    imgdir.mkdir(parents=True)
    rng = np.random.default_rng(23)
    for k in range(5):
        a = F.content("noise" if k % 2 else "ramp", 64, 96, 1, rng)[..., 0]
        (imgdir / f"img_{k}.png").write_bytes(F.write("grey", 64, 96, 90, "noise", rng) if k in (1, 4) else _png(a))
    kw = dict(save_npy=True, count_predictions=True, batch_size=3, obj_thresh=0.4, iou_thresh=0.5, class_names=CLASSES)
    predict(str(pth), path_to_images=imgdir, output_dir=str(tmp_path / "host"), **kw)
    host_out = capsys.readouterr().out
    _hip.launch_log(True)
    try:
        predict(str(pth), path_to_images=imgdir, output_dir=str(tmp_path / "dev"), device_image_decode=True, device_image_decode_jpeg=True, **kw)
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    assert capsys.readouterr().out == host_out and "you" in host_out
    a, b = sorted((tmp_path / "host").glob("*.npy")), sorted((tmp_path / "dev").glob("*.npy"))
    assert len(a) == 1 and [p.name for p in a] == [p.name for p in b] and a[0].read_bytes() == b[0].read_bytes()
    assert np.load(a[0]).shape[1] > 0
    assert sum(ln.startswith("jpeg_decode_kernel") for ln in log) == 2   # batches of 3 and 2: a JPEG in each
    with pytest.raises(ValueError, match="needs device_image_decode"):
        predict(str(pth), path_to_images=imgdir, device_image_decode_jpeg=True)
