"""The device image cache filled with files of ANOTHER size resized on the device (`yogo train --device-image-cache GIB
--device-image-decode --device-image-resize`; yogo_amd/png_prefill.py, csrc/resize_aa.hip) against the host prefill on the MI355X.

The dataset: 9 files for a cache of 24 x 33 -- grey and RGB ones at 35 x 20 (down in y, up in x) and at 48 x 70 (2 x and 2.1 x down),
three at the cache's own size, and an interlaced one at 48 x 70, which the device does not decode and the host resizes.  The resized
images are held to the fp64 oracle of tests/_resize_ref.py on the pixels ``read_image`` gives (the colour conversion comes before the
resize on both routes): rule H, which ``resize_image`` itself is held to; images that are not resized are bit-equal."""
from pathlib import Path

import numpy as np
import pytest
import torch

import _resize_ref as R
from _image_cache_data import write_defn
from _png_write import adam7_scan, png_bytes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HW = (24, 33)
Sx, Sy = 12, 8
CLASSES = ["you", "only", "glance", "once"]
# per file: (height, width), RGB?, interlaced?
FILES = [((35, 20), False, False), ((35, 20), True, False), ((48, 70), False, False), ((48, 70), True, False), (HW, False, False),
         (HW, True, False), ((48, 70), False, True), ((35, 20), False, False), (HW, False, False)]
N = len(FILES)
RESIZED = [k for k, (hw, _, lace) in enumerate(FILES) if hw != HW and not lace]
LACED = [k for k, (_, _, lace) in enumerate(FILES) if lace]


def _dataset(root: Path):
    img_dir, lab_dir = root / "images", root / "labels"
    img_dir.mkdir(parents=True)
    lab_dir.mkdir(parents=True)
    rng = np.random.default_rng(33)
    for k, ((h, w), rgb, lace) in enumerate(FILES):
        px = rng.integers(0, 256, size=(h, w, 3) if rgb else (h, w), dtype=np.uint8)
        if lace:
            data = png_bytes(px, scan=adam7_scan(px), ihdr=(w, h, 8, 0, 0, 0, 1))
        else:
            data = png_bytes(px, [int(t) for t in rng.integers(0, 5, size=h)], idat_sizes=[97, 201] if k % 2 else None)
        (img_dir / f"img_{k:04d}.png").write_bytes(data)
        lines = [f"{int(rng.integers(0, len(CLASSES)))} {rng.uniform(0.05, 0.95):.6f} {rng.uniform(0.05, 0.95):.6f} "
                 f"{rng.uniform(0.05, 0.3):.6f} {rng.uniform(0.05, 0.3):.6f}" for _ in range(2 + k % 3)]
        (lab_dir / f"img_{k:04d}.txt").write_text("".join(ln + "\n" for ln in lines))
    return img_dir, lab_dir


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = tmp_path_factory.mktemp("prefill_resize")
    img_dir, lab_dir = _dataset(root / "data")
    return root, img_dir, lab_dir


def _split(data, rgb):
    from yogo_amd.yogo_dataset import ObjectDetectionDataset

    _, img_dir, lab_dir = data
    split = ObjectDetectionDataset(img_dir, lab_dir, Sx, Sy, CLASSES, image_hw=HW, rgb=rgb)
    assert len(split) == N
    return split


def _exact(split, rgb):
    """the oracle's value of every sample's image: float64 [N, C, *HW] (the files at the cache's size: their pixels)"""
    from yogo_amd.yogo_dataset import read_image

    return np.stack([R.exact(read_image(str(split._image_paths[k]), rgb=rgb).numpy(), HW) for k in range(N)])


def _cache(split, rgb, **kw):
    from yogo_amd.image_cache import ImageCache

    c = ImageCache(split, N, (3 if rgb else 1, *HW), False, device=DEV, num_workers=0, batch_size=4, decode_batch=4, **kw)
    c.images.fill_(0x5A)
    c.prefill()
    return c


@pytest.mark.parametrize("rgb", [False, True])
def test_cache_with_device_resize_against_the_host_route(data, rgb):
    split = _split(data, rgb)
    v = _exact(split, rgb)
    R.assert_cap(v[RESIZED + LACED])
    host = _cache(split, rgb)
    dev = _cache(split, rgb, device_decode=True, device_resize=True)
    assert host.resident.all() and np.array_equal(dev.resident, host.resident)
    assert torch.equal(dev.rows, host.rows) and dev.rows.dtype == host.rows.dtype and np.array_equal(dev.row_offsets, host.row_offsets)
    hi, di = host.images.cpu().numpy(), dev.images.cpu().numpy()
    same = [k for k in range(N) if k not in RESIZED]
    assert np.array_equal(di[same], hi[same])   # the files at the cache's size, and the interlaced one the host resized on both routes
    R.assert_rule(hi[RESIZED + LACED], v[RESIZED + LACED], R.TOL_TORCH, "host cache")
    R.assert_rule(di[RESIZED], v[RESIZED], R.TOL_TORCH, "device cache")
    R.assert_rule(di[RESIZED], v[RESIZED], R.TOL_FP32, "device cache, the kernel's own rule")
    firm = R.edge_distance(v[RESIZED]) >= R.TOL_TORCH
    d = np.abs(di[RESIZED].astype(np.int64) - hi[RESIZED])
    print(f"device cache against host cache: {int((d != 0).sum())} of {d.size} resized pixels differ")
    assert not d[firm].any() and int(d.max()) <= 1
    st = dev.decode_stats
    assert st["device_resized"] == len(RESIZED) and st["host_decoded"] == len(LACED)
    # three chunks of 4, 4 and 1; per chunk one resize launch per file size in it: 35 x 20 and 48 x 70, 35 x 20, none
    assert len(st["unpack_ms"]) == 3 and len(st["resize_ms"]) == 3
    assert st["scratch_device_bytes"] > 0 and dev.full


@pytest.mark.parametrize("rgb", [False, True])
def test_cache_without_the_flag_is_todays(data, rgb):
    split = _split(data, rgb)
    host = _cache(split, rgb)
    dev = _cache(split, rgb, device_decode=True)
    assert torch.equal(dev.images, host.images) and torch.equal(dev.rows, host.rows) and np.array_equal(dev.row_offsets, host.row_offsets)
    assert dev.decode_stats["device_resized"] == 0 and dev.decode_stats["resize_ms"] == []
    assert dev.decode_stats["host_decoded"] == len(RESIZED) + len(LACED)
    again = _cache(split, rgb, device_decode=True, device_resize=False)
    assert torch.equal(again.images, host.images) and again.decode_stats["device_resized"] == 0


def test_the_flag_needs_device_decode(data):
    with pytest.raises(ValueError, match="needs --device-image-decode"):
        _cache(_split(data, False), False, device_resize=True)


@pytest.mark.parametrize("rgb", [False, True])
def test_first_epoch_with_and_without_the_flag(data, rgb):
    """the same labels; every image of a batch with the flag under rule H against the oracle's value of the sample it shows, which
    the batch without the flag identifies (that cache is the host's, bit for bit; the loader flips whole batches)"""
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.yogo_dataloader import get_dataloader

    root, img_dir, lab_dir = data
    split = _split(data, rgb)
    v = _exact(split, rgb)
    host = np.stack([split.image_uint8(k).numpy() for k in range(N)])
    defn = DatasetDefinition.from_yaml(write_defn(root, img_dir, lab_dir))
    epochs = {}
    for flag in (False, True):
        dls = get_dataloader(defn, 4, Sx, Sy, training=True, image_hw=HW, rgb=rgb, device=DEV, device_image_cache_gib=1.0,
                             device_image_decode=True, device_image_resize=flag)
        assert dls["train"].cache.device_resize is flag and dls["val"].cache.device_resize is flag
        res = {}
        for name in ("train", "val"):
            dls[name].sampler.set_epoch(0)
            torch.manual_seed(0)
            res[name] = [(i.cpu().numpy(), l.cpu()) for i, l in dls[name]]
        epochs[flag] = res
    flips = [lambda a: a, lambda a: a[..., ::-1], lambda a: a[..., ::-1, :], lambda a: a[..., ::-1, ::-1]]
    seen = set()
    for name in ("train", "val"):
        assert len(epochs[True][name]) == len(epochs[False][name]) > 0
        for (gi, gl), (wi, wl) in zip(epochs[True][name], epochs[False][name]):
            assert gi.dtype == wi.dtype and gi.shape == wi.shape and torch.equal(gl, wl), name
            for g, w in zip(gi, wi):
                k, flip = next((k, f) for k in range(N) for f in flips if np.array_equal(f(host[k]), w))
                seen.add(k)
                if k in RESIZED:
                    R.assert_rule(g, flip(v[k]), R.TOL_TORCH, f"{name} sample {k}")
                else:
                    assert np.array_equal(g, w)
    assert seen == set(range(N))
