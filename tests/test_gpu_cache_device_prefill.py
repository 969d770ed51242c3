"""The device image cache filled by the device decoder (yogo_amd/png_prefill.py, `yogo train --device-image-cache GIB
--device-image-decode`) against the host prefill on the MI355X: the same cache, the same batches, the global RNG untouched,
and `train` end to end in a child process.

The dataset: 11 images at 70 x 37 -- grey and RGB files with mixed filters, which the device decodes whatever the model's channel
count, and everything the device hands to the host: an interlaced file, a 16-bit one, a palette one, one at 35 x 20 (resized), a
JPEG under a .png name, a truncated file (unreadable on both routes) -- with label files of 0, 1 and several lines.  The loader's
csv sniffer takes the only line of a one-line file for a header (as the reference's does), so those load as no row; sample 6 has
two lines of which the area filter keeps one, so that a sample of exactly one row is there as well."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from _image_cache_data import write_defn
from _png_write import adam7_scan, png_bytes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEV = torch.device("cuda", 0)
HW = (70, 37)
Sx, Sy = 12, 8
N = 11
CLASSES = ["you", "only", "glance", "once"]


def _dataset(root: Path):
    from PIL import Image

    img_dir, lab_dir = root / "images", root / "labels"
    img_dir.mkdir(parents=True)
    lab_dir.mkdir(parents=True)
    rng = np.random.default_rng(21)
    H, W = HW

    def grey(hw=HW):
        return rng.integers(0, 256, size=hw, dtype=np.uint8)

    def rgb():
        return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)

    def mixed():
        return [int(t) for t in rng.integers(0, 5, size=H)]

    files = [
        png_bytes(grey(), mixed()),
        png_bytes(rgb(), mixed(), idat_sizes=[100, 333]),
        png_bytes(grey(), mixed(), idat_sizes=[1, 2, 3]),
        png_bytes(rgb(), mixed()),
        png_bytes(grey(), [4] * H, level=0),
    ]
    lace = grey()
    files.append(png_bytes(lace, scan=adam7_scan(lace), ihdr=(W, H, 8, 0, 0, 0, 1)))                      # interlaced
    for k, data in enumerate(files):
        (img_dir / f"img_{k:04d}.png").write_bytes(data)
    Image.fromarray(rng.integers(0, 65536, size=HW, dtype=np.uint16)).save(img_dir / "img_0006.png")       # 16-bit
    Image.fromarray(grey()).convert("P").save(img_dir / "img_0007.png")                                    # palette
    (img_dir / "img_0008.png").write_bytes(png_bytes(grey((35, 20)), [int(t) for t in rng.integers(0, 5, size=35)]))   # resized
    Image.fromarray(rgb()).save(img_dir / "img_0009.png", format="JPEG")                                   # a JPEG under a .png name
    whole = png_bytes(grey(), mixed())
    (img_dir / "img_0010.png").write_bytes(whole[:len(whole) // 2])                                        # truncated
    for k in range(N):
        m = (0, 1, 4, 2, 0, 3, 1, 5, 2, 1, 3)[k]
        lines = [f"{int(rng.integers(0, len(CLASSES)))} {rng.uniform(0.05, 0.95):.6f} {rng.uniform(0.05, 0.95):.6f} "
                 f"{rng.uniform(0.05, 0.3):.6f} {rng.uniform(0.05, 0.3):.6f}" for _ in range(m)]
        if k == 6:
            lines.append("2 0.500000 0.500000 0.010000 0.010000")   # under the area filter: the sample loads as one row
        (lab_dir / f"img_{k:04d}.txt").write_text("".join(ln + "\n" for ln in lines))
    return img_dir, lab_dir


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = tmp_path_factory.mktemp("prefill")
    img_dir, lab_dir = _dataset(root / "data")
    return root, img_dir, lab_dir


@pytest.mark.filterwarnings("ignore:could not read")
@pytest.mark.parametrize("rgb", [False, True])
def test_cache_equal_on_both_routes(data, rgb):
    from yogo_amd.image_cache import ImageCache
    from yogo_amd.yogo_dataset import ObjectDetectionDataset

    _, img_dir, lab_dir = data
    split = ObjectDetectionDataset(img_dir, lab_dir, Sx, Sy, CLASSES, image_hw=HW, rgb=rgb)
    assert len(split) == N
    caches = {}
    for flag in (False, True):
        c = ImageCache(split, N, (3 if rgb else 1, *HW), False, device=DEV, num_workers=0, batch_size=4, device_decode=flag, decode_batch=3)
        c.images.fill_(0x5A)
        torch.manual_seed(1234)
        before = torch.get_rng_state()
        c.prefill()
        assert torch.equal(torch.get_rng_state(), before), flag
        caches[flag] = c
    host, dev = caches[False], caches[True]
    assert host.resident.tolist() == [True] * (N - 1) + [False]           # the truncated file alone is unreadable
    assert np.array_equal(dev.resident, host.resident)
    assert torch.equal(dev.images.cpu(), host.images.cpu())              # (the slot of the unreadable file: untouched on both)
    assert torch.equal(dev.rows, host.rows) and dev.rows.dtype == host.rows.dtype
    assert np.array_equal(dev.row_offsets, host.row_offsets)
    assert dev.row_offsets[-1] == dev.rows.shape[0] > 0 and {0, 1, 4} <= set(np.diff(dev.row_offsets).tolist())   # 0, 1 and several rows
    # four chunks of 3, 3, 3 and 2; the device decoded the five plain files and nothing else
    assert len(dev.decode_stats["unpack_ms"]) == 4 and dev.decode_stats["host_decoded"] == 6
    assert dev.full is False and dev.prefilled


@pytest.mark.filterwarnings("ignore:could not read")
@pytest.mark.parametrize("rgb", [False, True])
def test_first_epoch_equal_with_and_without_the_flag(data, rgb):
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.yogo_dataloader import get_dataloader

    root, img_dir, lab_dir = data
    defn = DatasetDefinition.from_yaml(write_defn(root, img_dir, lab_dir))
    epochs = {}
    for flag in (False, True):
        dls = get_dataloader(defn, 4, Sx, Sy, training=True, image_hw=HW, rgb=rgb, device=DEV, device_image_cache_gib=1.0,
                             device_image_decode=flag)
        assert dls["train"].cache.device_decode is flag and dls["val"].cache.device_decode is flag
        res = {}
        for name in ("train", "val"):
            dls[name].sampler.set_epoch(0)
            torch.manual_seed(0)
            res[name] = [(i.cpu(), l.cpu()) for i, l in dls[name]]
        epochs[flag] = res
    for name in ("train", "val"):
        assert len(epochs[True][name]) == len(epochs[False][name]) > 0
        for (gi, gl), (wi, wl) in zip(epochs[True][name], epochs[False][name]):
            assert gi.dtype == wi.dtype and torch.equal(gi, wi) and torch.equal(gl, wl), name


def test_the_flag_needs_a_cache(data):
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.yogo_dataloader import get_dataloader

    root, img_dir, lab_dir = data
    defn = DatasetDefinition.from_yaml(write_defn(root, img_dir, lab_dir))
    with pytest.raises(ValueError, match="device-image-cache"):
        get_dataloader(defn, 4, Sx, Sy, image_hw=HW, device=DEV, device_image_decode=True)


def test_train_with_the_flag_in_a_child_process(data, tmp_path):
    """`train <defn> --device-image-cache 1 --device-image-decode -bs 4 --epochs 1` at the files' own size (at the default
    --image-hw every file would be resized on the host and the device would decode nothing), under a run name"""
    root, img_dir, lab_dir = data
    defn = write_defn(root, img_dir, lab_dir)
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "yogo_amd", "train", str(defn), "--device-image-cache", "1", "--device-image-decode", "-bs", "4",
                        "--epochs", "1", "--image-hw", str(HW[0]), str(HW[1]), "--name", "prefill_cli"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device image cache (train)" in r.stdout and (tmp_path / "trained_models" / "prefill_cli" / "best.pth").exists()
