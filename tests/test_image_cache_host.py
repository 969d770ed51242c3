"""Host side of the device image cache (yogo_amd/image_cache.py, `yogo train --device-image-cache GIB`): the budget -> S
arithmetic, the refused budgets, the flag's default and its way into the config, the budget split between train and val, the
worker-side wrapper (markers for resident indices, the plain dataset's bits for the others, None for an unreadable file,
pickling) and the collate.  No GPU needed."""
import math
import pickle

import numpy as np
import pytest
import torch
from torch.utils.data import ConcatDataset, Subset

from _image_cache_data import CLASSES, write_defn, write_images


def test_budget_to_resident_count():
    from yogo_amd.image_cache import GIB, budget_bytes, resident_count

    per1, per3 = 772 * 1032, 3 * 772 * 1032
    assert per1 == 796704 and per1 % 16 == 0   # (the gather's 16-byte path applies at the production size)
    assert budget_bytes(1) == GIB and budget_bytes(0.5) == GIB // 2 and budget_bytes(1.5) == 3 * GIB // 2
    # floor(budget / (C * H * W)), capped by the split size
    assert resident_count(budget_bytes(1), 10 ** 6, 1, 772, 1032) == GIB // per1 == 1347
    assert resident_count(budget_bytes(1), 10 ** 6, 3, 772, 1032) == GIB // per3 == 449
    assert resident_count(budget_bytes(200), 10 ** 6, 1, 772, 1032) == 200 * GIB // per1
    assert resident_count(budget_bytes(1), 100, 1, 772, 1032) == 100
    assert resident_count(budget_bytes(1), 100, 3, 772, 1032) == 100
    assert resident_count(per1 - 1, 100, 1, 772, 1032) == 0
    assert resident_count(per1, 100, 1, 772, 1032) == 1
    assert resident_count(per3 * 7 + per3 - 1, 100, 3, 772, 1032) == 7
    assert resident_count(10 * 3 * 96 * 128, 100, 3, 96, 128) == 10


@pytest.mark.parametrize("bad", ["0", "-1", "-0.5", "nan", "NaN", "inf", "abc"])
def test_refused_budgets(bad):
    from yogo_amd.image_cache import check_budget_gib
    from yogo_amd.utils.argparsers import global_parser

    with pytest.raises(SystemExit):
        global_parser().parse_args(["train", "defn.yml", "--device-image-cache", bad])
    with pytest.raises(ValueError):
        check_budget_gib(float(bad) if bad != "abc" else bad)


def test_flag_default_and_config():
    from yogo_amd.trainer import build_config
    from yogo_amd.utils.argparsers import global_parser

    args = global_parser().parse_args(["train", "defn.yml"])
    assert args.device_image_cache is None and build_config(args)["device_image_cache_gib"] is None
    args = global_parser().parse_args(["train", "defn.yml", "--device-image-cache", "2.5"])
    assert args.device_image_cache == 2.5 and build_config(args)["device_image_cache_gib"] == 2.5


def test_get_dataloader_refuses_bad_budget(tmp_path):
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.yogo_dataloader import get_dataloader

    defn = DatasetDefinition.from_yaml(write_defn(tmp_path, *write_images(tmp_path / "d", 4)))
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="device-image-cache"):
            get_dataloader(defn, 2, 12, 8, image_hw=(64, 96), device_image_cache_gib=bad)


class _RecordingCache:
    """stands in for ImageCache (which allocates on the device): records what get_dataloader asks for"""
    made = []

    def __init__(self, split, S, image_shape, normalize_images, device=None, num_workers=0, batch_size=64, name="train", log=False):
        self.S, self.image_shape, self.name, self.split = S, image_shape, name, split
        self.resident = np.zeros(S, dtype=bool)
        _RecordingCache.made.append(self)


@pytest.mark.parametrize("rgb", [False, True])
def test_budget_covers_train_first_then_val(tmp_path, monkeypatch, rgb):
    import yogo_amd.yogo_dataloader as ydl
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.image_cache import ResidentMarkers

    img_dir, lab_dir = write_images(tmp_path / "d", 20, hw=(64, 96), rgb=rgb)
    defn_path = tmp_path / "defn.yml"
    defn_path.write_text("class_names: [you, only, glance, once]\n"
                         "dataset_split_fractions: {train: 0.5, val: 0.25, test: 0.25}\n"
                         f"dataset_paths:\n  a: {{image_path: {img_dir}, label_path: {lab_dir}}}\n")
    defn = DatasetDefinition.from_yaml(defn_path)
    monkeypatch.setattr(ydl, "ImageCache", _RecordingCache)
    per = (3 if rgb else 1) * 64 * 96
    for images, want in ((3, {"train": 3}), (10, {"train": 10}), (13, {"train": 10, "val": 3}), (100, {"train": 10, "val": 5})):
        _RecordingCache.made = []
        d = ydl.get_dataloader(defn, 4, 12, 8, image_hw=(64, 96), rgb=rgb, device_image_cache_gib=images * per / 2 ** 30)
        assert {c.name: c.S for c in _RecordingCache.made} == want, images
        assert all(c.image_shape == ((3 if rgb else 1), 64, 96) for c in _RecordingCache.made)
        for name in ("train", "val", "test"):
            cached = name in want
            assert isinstance(d[name].loader.dataset, ResidentMarkers) == cached
            assert (d[name].cache is not None) == cached
            assert isinstance(d[name].dataset, Subset)   # the split as get_datasets made it, cached or not
    # no flag: the loaders of today -- no cache object, the plain split in the DataLoader
    _RecordingCache.made = []
    d = ydl.get_dataloader(defn, 4, 12, 8, image_hw=(64, 96), rgb=rgb)
    assert not _RecordingCache.made and all(dl.cache is None and isinstance(dl.loader.dataset, Subset) for dl in d.values())
    # a budget smaller than one image caches nothing
    d = ydl.get_dataloader(defn, 4, 12, 8, image_hw=(64, 96), rgb=rgb, device_image_cache_gib=(per - 1) / 2 ** 30)
    assert not _RecordingCache.made and all(dl.cache is None for dl in d.values())


def _dataset(tmp_path, normalize: bool, truncated=()):
    from yogo_amd.yogo_dataset import ObjectDetectionDataset

    img_dir, lab_dir = write_images(tmp_path / f"d{int(normalize)}", 6, hw=(64, 96), truncated=truncated)
    return ObjectDetectionDataset(img_dir, lab_dir, 12, 8, CLASSES, image_hw=(64, 96), normalize_images=normalize)


@pytest.mark.parametrize("normalize", [False, True])
def test_worker_wrapper(tmp_path, normalize):
    from yogo_amd.image_cache import ResidentIndex, ResidentMarkers, resolve_sample

    ods = _dataset(tmp_path, normalize, truncated=[4])
    split = Subset(ConcatDataset([ods]), [5, 3, 1, 0, 4, 2])
    resident = np.array([True, False, True])   # split indices 0 and 2 are resident, 1 is not (unreadable at prefill, say)
    w = ResidentMarkers(split, resident)
    assert len(w) == len(split) == 6
    for i in (0, 2):
        m = w[i]
        assert isinstance(m, ResidentIndex) and int(m) == i
    for i in (1, 3, 5):
        img, rows = w[i]
        want_img, want_rows = split[i]
        assert img.dtype == (torch.float32 if normalize else torch.uint8) and torch.equal(img, want_img) and torch.equal(rows, want_rows)
    with pytest.warns(UserWarning, match="could not read"):
        assert w[4] is None   # split index 4 -> file 4, truncated
    # the accessor the prefill uses: the uint8 image before normalize_images' / 255, resolved through Subset / ConcatDataset
    for i in (0, 1, 3):
        ds, j = resolve_sample(split, i)
        assert ds is ods and j == [5, 3, 1, 0, 4, 2][i]
        u8 = ds.image_uint8(j)
        assert u8.dtype == torch.uint8 and torch.equal(u8 / 255 if normalize else u8, split[i][0])
    # spawn workers receive a pickled copy
    w2 = pickle.loads(pickle.dumps(w))
    assert isinstance(w2[0], ResidentIndex) and int(w2[2]) == 2 and torch.equal(w2[1][0], w[1][0])
    assert pickle.loads(pickle.dumps(ResidentIndex(7))) == 7 and isinstance(pickle.loads(pickle.dumps(ResidentIndex(7))), ResidentIndex)


def test_collate_cached():
    from yogo_amd.image_cache import ResidentIndex, collate_cached

    a, b = torch.full((1, 4, 6), 3, dtype=torch.uint8), torch.full((1, 4, 6), 9, dtype=torch.uint8)
    ra, rb = torch.rand(2, 5), torch.rand(0, 5)
    batch = [None, ResidentIndex(4), (a, ra), 7, None, ResidentIndex(0), (b, rb), 2]
    imgs, rows, up_pos, res_idx, res_pos, blob_idx, blob_pos, B = collate_cached(batch)
    assert B == 6 and up_pos == [1, 4] and res_idx == [4, 0] and res_pos == [0, 3] and blob_idx == [7, 2] and blob_pos == [2, 5]
    assert torch.equal(imgs, torch.stack([a, b])) and rows[0] is ra and rows[1] is rb
    assert all(type(i) is int for i in res_idx + blob_idx)
    # only markers: no image tensor; nothing left: None
    imgs, rows, up_pos, res_idx, res_pos, _, _, B = collate_cached([ResidentIndex(3), None, ResidentIndex(1)])
    assert imgs is None and rows == [] and up_pos == [] and res_idx == [3, 1] and res_pos == [0, 1] and B == 2
    assert collate_cached([None, None]) is None


def test_gather_refuses_host_tensors():
    from yogo_amd.image_cache import gather

    with pytest.raises(RuntimeError, match="MI355X"):
        gather(torch.zeros(2, 1, 4, 4, dtype=torch.uint8), [0], torch.zeros(1, 1, 4, 4, dtype=torch.uint8))
