"""Labelled batches decoded on the device every epoch (``device_image_stream``, yogo_amd/image_stream.py) against the worker route on
the MI355X: the same sequence of ``(imgs, labels)`` -- dtype, shape and bits -- without a cache, beside a partial cache, with blob
rows, on two ranks and after an abandoned iteration; what the device really decoded; the resize route; unreadable files; the global
RNG; no workers; and ``yogo test`` / ``yogo train`` with the flag in child processes.

The dataset: 23 images at 70 x 37 (train 17, val 6) -- 17 plain grey and RGB files with mixed filters, which the device decodes, and
the six of tests/test_gpu_cache_device_prefill.py that it hands to the host: interlaced, 16-bit, palette, one at 35 x 20, a JPEG under a
.png name, a truncated file (unreadable on every route).  Batch 4: the train split is batches of 4, 4, 4, 4 and 1.  With
``stream_decode_batch`` 9 that is a group of two batches (8 samples) and one of three (8 + 1 = 9 fit): a group boundary mid-epoch and a
partial last batch; with 8 the groups are 2, 2 and 1 batches, the last group partial as well; 1 makes every batch a group that ``fill``
chunks, 1 000 the epoch one group."""
import os
import pickle
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _resize_ref as R
from _png_write import adam7_scan, png_bytes

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:could not read")]
ROOT = Path(__file__).resolve().parent.parent
DEV = torch.device("cuda", 0)
HW = (70, 37)
Sx, Sy = 12, 8
N = 23
CLASSES = ["you", "only", "glance", "once"]
ODD = {17: "interlaced", 18: "16-bit", 19: "palette", 20: "35 x 20", 21: "jpeg", 22: "truncated"}
SMALL, JPEG, TRUNCATED = 20, 21, 22
BS, DB = 4, 9


def _dataset(root: Path):
    from PIL import Image

    img_dir, lab_dir = root / "images", root / "labels"
    img_dir.mkdir(parents=True)
    lab_dir.mkdir(parents=True)
    rng = np.random.default_rng(77)
    H, W = HW

    def grey(hw=HW):
        return rng.integers(0, 256, size=hw, dtype=np.uint8)

    def rgb():
        return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)

    def mixed(h=H):
        return [int(t) for t in rng.integers(0, 5, size=h)]

    for k in range(17):
        data = png_bytes(rgb() if k % 3 == 1 else grey(), mixed(), idat_sizes=[100, 333] if k % 4 == 2 else None)
        (img_dir / f"img_{k:04d}.png").write_bytes(data)
    lace = grey()
    (img_dir / "img_0017.png").write_bytes(png_bytes(lace, scan=adam7_scan(lace), ihdr=(W, H, 8, 0, 0, 0, 1)))
    Image.fromarray(rng.integers(0, 65536, size=HW, dtype=np.uint16)).save(img_dir / "img_0018.png")
    Image.fromarray(grey()).convert("P").save(img_dir / "img_0019.png")
    (img_dir / "img_0020.png").write_bytes(png_bytes(grey((35, 20)), mixed(35)))
    Image.fromarray(rgb()).save(img_dir / "img_0021.png", format="JPEG")
    whole = png_bytes(grey(), mixed())
    (img_dir / "img_0022.png").write_bytes(whole[:len(whole) // 2])
    for k in range(N):
        m = (0, 2, 4, 3, 0, 5)[k % 6]
        lines = [f"{int(rng.integers(0, len(CLASSES)))} {rng.uniform(0.05, 0.95):.6f} {rng.uniform(0.05, 0.95):.6f} "
                 f"{rng.uniform(0.05, 0.3):.6f} {rng.uniform(0.05, 0.3):.6f}" for _ in range(m)]
        (lab_dir / f"img_{k:04d}.txt").write_text("".join(ln + "\n" for ln in lines))
    return img_dir, lab_dir


def _defn_text(img_dir, lab_dir, thumbnails=None, test_paths=None) -> str:
    text = ("class_names: [you, only, glance, once]\n"
            "dataset_split_fractions: {train: 0.75, val: 0.25}\n"
            f"dataset_paths:\n  a: {{image_path: {img_dir}, label_path: {lab_dir}}}\n")
    if test_paths:
        text += f"test_paths:\n  t: {{image_path: {test_paths / 'images'}, label_path: {test_paths / 'labels'}}}\n"
    if thumbnails:
        text += "thumbnail_augmentation:\n" + "".join(f"  {k}: {v}\n" for k, v in thumbnails.items())
    return text


def _thumbs(root: Path) -> dict:
    from PIL import Image

    rng = np.random.default_rng(11)
    out = {}
    for name, dims in (("glance", [(24, 24), (25, 30)]), ("once", [(22, 28), (26, 26)])):
        d = root / name
        d.mkdir(parents=True, exist_ok=True)
        for k, (h, w) in enumerate(dims):
            Image.fromarray(np.clip(rng.normal(200, 30, size=(h, w)), 0, 255).astype(np.uint8), mode="L").save(d / f"t{k}.png")
        out[name] = d
    return out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from yogo_amd.dataset_definition_file import DatasetDefinition

    root = tmp_path_factory.mktemp("stream")
    img_dir, lab_dir = _dataset(root / "data")
    shutil.copytree(root / "data", root / "held_out")   # (a test set must not be the training set's folders)
    paths = {}
    for name, kw in (("plain", {}), ("thumbs", {"thumbnails": _thumbs(root / "thumbs")}), ("test", {"test_paths": root / "held_out"})):
        paths[name] = root / f"{name}.yml"
        paths[name].write_text(_defn_text(img_dir, lab_dir, **kw))
    return root, img_dir, lab_dir, paths, {k: DatasetDefinition.from_yaml(p) for k, p in paths.items()}


def _loaders(data, defn="plain", **kw):
    from yogo_amd.yogo_dataloader import get_dataloader

    kw.setdefault("training", True)
    if kw.get("device_image_stream"):
        kw.setdefault("stream_decode_batch", DB)
    return get_dataloader(data[4][defn], kw.pop("bs", BS), Sx, Sy, image_hw=HW, device=DEV, **kw)


def _run(dls, epochs=(0, 1), names=("train", "val")):
    """{split: [epoch][batch] (imgs, labels) on the host}: set_epoch and torch.manual_seed before every epoch (val: epoch 0 alone)"""
    out = {}
    for name in names:
        res = []
        for e in (epochs if name == "train" else epochs[:1]):
            dls[name].sampler.set_epoch(e)
            torch.manual_seed(100 + e)
            res.append([(i.cpu(), l.cpu()) for i, l in dls[name]])
        out[name] = res
    return out


def _close(dls):
    for dl in dls.values():
        if dl.stream is not None:
            dl.stream.scratch.close()


def _assert_same(got, want):
    assert got.keys() == want.keys()
    for name in got:
        assert len(got[name]) == len(want[name]) > 0
        for e, (ge, we) in enumerate(zip(got[name], want[name])):
            assert len(ge) == len(we) > 0, (name, e, len(ge), len(we))
            for k, ((gi, gl), (wi, wl)) in enumerate(zip(ge, we)):
                assert gi.dtype == wi.dtype and gi.shape == wi.shape and torch.equal(gi, wi), (name, e, k)
                assert gl.dtype == wl.dtype and gl.shape == wl.shape and torch.equal(gl, wl), (name, e, k)


_WORKERS = {}


@pytest.fixture
def workers(data):
    """the worker route's batches, computed once per (definition, rgb) and shared"""
    def get(defn="plain", rgb=False):
        if (defn, rgb) not in _WORKERS:
            _WORKERS[defn, rgb] = _run(_loaders(data, defn, rgb=rgb))
        return _WORKERS[defn, rgb]
    return get


def _file_of(dataset, i: int) -> int:
    """the number of the file behind split index i"""
    from yogo_amd.image_cache import resolve_sample

    ds, j = resolve_sample(dataset, i)
    return int(Path(str(ds._image_paths[j])).stem.split("_")[1])


@pytest.mark.parametrize("decode_batch", [DB, 8, 1, 1000])
@pytest.mark.parametrize("rgb", [False, True])
def test_no_cache_equals_the_worker_route(data, workers, rgb, decode_batch):
    dls = _loaders(data, rgb=rgb, device_image_stream=True, stream_decode_batch=decode_batch)
    assert dls["train"].cache is None and dls["train"].stream.scratch is dls["val"].stream.scratch
    assert len(dls["train"].dataset) == 17 and len(dls["val"].dataset) == 6
    got = _run(dls)
    _assert_same(got, workers(rgb=rgb))
    assert got["train"][0][0][0].dtype == torch.uint8 and got["train"][0][0][0].shape[1] == (3 if rgb else 1)
    st = dls["train"].stream.stats
    per_epoch = {DB: 2, 8: 3, 1: 5, 1000: 1}[decode_batch]
    assert st["groups"] == 2 * per_epoch and st["streamed"] == 2 * 17 and dls["val"].stream.stats["streamed"] == 6
    assert st["hbm_bytes"] >= 2 * max(decode_batch, BS) * (3 if rgb else 1) * HW[0] * HW[1] and st["pinned_bytes"] > 0
    sc = dls["train"].stream.scratch
    sc.close()
    assert sc.filler is None and sc.staging == [] and sc.hbm_bytes == 0


def test_normalized_images_equal_the_worker_route(data):
    want = _run(_loaders(data, normalize_images=True), epochs=(0,))
    dls = _loaders(data, normalize_images=True, device_image_stream=True)
    got = _run(dls, epochs=(0,))
    _assert_same(got, want)
    assert got["train"][0][0][0].dtype == torch.float32
    _close(dls)


def test_partial_cache_equals_the_same_cache_without_the_stream(data):
    gib = 5.5 * HW[0] * HW[1] / 2 ** 30   # five images and a half: five train samples resident, nothing left for val
    plain = _loaders(data, device_image_cache_gib=gib)
    dls = _loaders(data, device_image_cache_gib=gib, device_image_stream=True)
    assert dls["train"].cache.S == 5 and dls["val"].cache is None and plain["train"].cache.S == 5
    got = _run(dls)
    _assert_same(got, _run(plain))
    resident = int(dls["train"].cache.resident.sum())
    assert resident == 5 - sum(_file_of(dls["train"].dataset, i) == TRUNCATED for i in range(5))
    assert dls["train"].stream.stats["streamed"] == 2 * (17 - resident) and dls["val"].stream.stats["streamed"] == 6
    _close(dls)


def test_thumbnail_augmentation_equals_the_worker_route(data, workers):
    dls = _loaders(data, "thumbs", device_image_stream=True)
    assert dls["train"].blob is not None and len(dls["train"].dataset) == 17 + 8
    _assert_same(_run(dls), workers("thumbs"))
    assert dls["train"].stream.stats["streamed"] == 2 * 17   # the blob indices are not decoded
    _close(dls)


def test_the_device_really_decoded(data):
    """every sample once (train and val, one epoch): the 17 plain files on the device, the six odd ones through the host decoder;
    with decode_all the host keeps what is no PNG (the JPEG), what does not parse (the truncated file) and -- without the resize
    switch, as in the prefill -- the file of another size; with both switches the JPEG and the truncated file alone"""
    from yogo_amd import _hip

    for kw, host, resized in (({}, 6, 0), ({"device_image_decode_all": True}, 3, 0),
                              ({"device_image_decode_all": True, "device_image_resize": True}, 2, 1)):
        dls = _loaders(data, training=False, device_image_stream=True, **kw)
        _hip.launch_log(True)
        _run(dls, epochs=(0,))
        log = _hip.read_launch_log()
        _hip.launch_log(False)
        stats = [dls[name].stream.stats for name in ("train", "val")]
        assert sum(s["streamed"] for s in stats) == N, kw
        assert sum(s["host_decoded"] for s in stats) == host, kw
        assert sum(s["device_resized"] for s in stats) == resized, kw
        assert sum(len(s["inflate_ms"]) for s in stats) == 3 and sum(len(s["unpack_ms"]) for s in stats) == 3   # groups of 8 + 9 and of 6
        assert sum(1 for ln in log if ln.startswith("inflate_zlib_kernel")) == 3, sorted({ln.split("|")[0] for ln in log})
        assert sum(1 for ln in log if ln.startswith("image_cache_gather")) == len(dls["train"]) + len(dls["val"])
        _close(dls)


def test_resize_holds_the_small_file_to_the_oracle(data, workers):
    """with device_image_resize the 35 x 20 file stays on the device: under rule H against the fp64 oracle, within one grey level of
    the worker route and equal wherever the exact value is not at a rounding edge; every other image bit-equal"""
    from yogo_amd.yogo_dataset import ObjectDetectionDataset, read_image

    _, img_dir, lab_dir = data[:3]
    files = ObjectDetectionDataset(img_dir, lab_dir, Sx, Sy, CLASSES, image_hw=HW)
    small = files.image_uint8(SMALL).numpy()
    v = R.exact(read_image(str(files._image_paths[SMALL])).numpy(), HW)
    R.assert_cap(v[None])
    want = _run(_loaders(data, training=False), epochs=(0,))
    dls = _loaders(data, training=False, device_image_stream=True, device_image_resize=True)
    got = _run(dls, epochs=(0,))
    seen = 0
    for name in ("train", "val"):
        assert len(got[name][0]) == len(want[name][0])
        for (gi, gl), (wi, wl) in zip(got[name][0], want[name][0]):
            assert gi.dtype == wi.dtype and gi.shape == wi.shape and torch.equal(gl, wl)
            for g, w in zip(gi.numpy(), wi.numpy()):
                if not np.array_equal(w, small):
                    assert np.array_equal(g, w)
                    continue
                seen += 1
                R.assert_rule(g, v, R.TOL_TORCH, "streamed 35 x 20 file")
                R.assert_rule(g, v, R.TOL_FP32, "streamed 35 x 20 file, the kernel's own rule")
                d = np.abs(g.astype(np.int64) - w)
                print(f"stream against workers: {int((d != 0).sum())} of {d.size} resized pixels differ")
                assert not d[R.edge_distance(v) >= R.TOL_TORCH].any() and int(d.max()) <= 1
    assert seen == 1
    assert dls["train"].stream.stats["device_resized"] + dls["val"].stream.stats["device_resized"] == 1
    _close(dls)


def test_unreadable_file_is_dropped_and_its_batch_closes_up(data, workers):
    want = workers()
    dls = _loaders(data, device_image_stream=True)
    split = "train" if any(_file_of(dls["train"].dataset, i) == TRUNCATED for i in range(17)) else "val"
    n = len(dls[split].dataset)
    got = _run(dls, names=(split,))
    for ge, we in zip(got[split], want[split]):
        assert sum(i.shape[0] for i, _ in ge) == n - 1 == sum(i.shape[0] for i, _ in we)
        assert [i.shape[0] for i, _ in ge] == [i.shape[0] for i, _ in we]
    _close(dls)
    # batch 1: the truncated file's batch is the None item, skipped on both routes
    one = _run(_loaders(data, bs=1), epochs=(0,))
    dls = _loaders(data, bs=1, device_image_stream=True)
    got = _run(dls, epochs=(0,))
    _assert_same(got, one)
    assert len(got["train"][0]) + len(got["val"][0]) == N - 1 and len(dls["train"]) + len(dls["val"]) == N
    _close(dls)


def test_label_file_that_does_not_parse_raises_at_its_batch(data, tmp_path):
    """the worker route raises from ``label_rows`` when it reaches the sample; so does the stream, after the batches before it"""
    from yogo_amd.dataset_definition_file import DatasetDefinition

    _, img_dir, lab_dir = data[:3]
    bad_labels = tmp_path / "labels"
    shutil.copytree(lab_dir, bad_labels)
    defn_path = tmp_path / "bad.yml"
    defn_path.write_text(_defn_text(img_dir, bad_labels))
    from yogo_amd.yogo_dataloader import get_dataloader

    defn = DatasetDefinition.from_yaml(defn_path)
    probe = get_dataloader(defn, BS, Sx, Sy, training=False, image_hw=HW, device=DEV)["train"]
    probe.sampler.set_epoch(0)
    order = [int(i) for i in probe.sampler]
    victim = next(f for f in (_file_of(probe.dataset, i) for i in order[8:12]) if f != TRUNCATED)   # in the third batch
    (bad_labels / f"img_{victim:04d}.txt").write_text("0 0.5 0.5 0.2 0.2\n1 0.4 0.4 0.2 0.2\n2 0.3 bad 0.2 0.2\n3 0.6 0.6 0.2 0.2\n")
    seen = {}
    for flag in (False, True):
        dl = get_dataloader(defn, BS, Sx, Sy, training=False, image_hw=HW, device=DEV, device_image_stream=flag, stream_decode_batch=DB)["train"]
        dl.sampler.set_epoch(0)
        n = 0
        with pytest.raises(RuntimeError, match="exception from") as e:
            for _ in dl:
                n += 1
        seen[flag] = (n, str(e.value))
        if flag:
            dl.stream.scratch.close()
    assert seen[True] == seen[False] and seen[True][0] == 2, seen


def test_global_rng_is_untouched(data):
    dls = _loaders(data, training=False, device_image_stream=True)
    torch.manual_seed(4321)
    before = torch.get_rng_state()
    for name in ("train", "val"):
        assert sum(1 for _ in dls[name]) == len(dls[name])
    assert torch.equal(torch.get_rng_state(), before)
    _close(dls)


class _NoIter:
    """a DataLoader that must never be iterated"""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        raise AssertionError("the stream route iterated the host DataLoader")


def test_stream_route_starts_no_workers(data, workers, monkeypatch):
    import yogo_amd.yogo_dataloader as ydl
    from torch.utils.data import DataLoader

    monkeypatch.setattr(ydl, "choose_dataloader_num_workers", lambda n, requested=None: 2)
    dls = _loaders(data, device_image_stream=True)
    for dl in dls.values():
        assert dl.loader.num_workers == 0
        dl.loader = _NoIter(dl.loader)

    def refuse(self):
        raise AssertionError("a DataLoader was iterated")

    monkeypatch.setattr(DataLoader, "__iter__", refuse)
    got = _run(dls)
    monkeypatch.undo()
    _assert_same(got, workers())
    _close(dls)


def test_two_ranks_equal_the_worker_route(data):
    """each rank's shard (23 samples on 2 ranks: 12 each, one padded duplicate) through ``_get_dataloader`` on both routes"""
    from yogo_amd.data import RandomHorizontalFlipWithBBs, RandomVerticalFlipWithBBs
    from yogo_amd.image_stream import Scratch
    from yogo_amd.yogo_dataloader import _get_dataloader, get_datasets

    split = torch.utils.data.ConcatDataset(list(get_datasets(data[4]["plain"], Sx, Sy, image_hw=HW).values()))
    assert len(split) == N
    sc = Scratch((1, *HW), BS, DB, DEV)
    orders = []
    for r in (0, 1):
        augs = [RandomHorizontalFlipWithBBs(0.5), RandomVerticalFlipWithBBs(0.5)]
        plain = _get_dataloader(split, BS, augs, r, 2, Sx, Sy, DEV, strict_steps=True)
        stream = _get_dataloader(split, BS, augs, r, 2, Sx, Sy, DEV, strict_steps=True, image_shape=(1, *HW), name=f"rank{r}", scratch=sc)
        assert len(plain.sampler) == 12 and stream.stream is not None
        _assert_same(_run({"train": stream}, names=("train",)), _run({"train": plain}, names=("train",)))
        orders.append([int(i) for i in stream.sampler])
    assert orders[0] != orders[1] and len(orders[0] + orders[1]) == 24 and len(set(orders[0] + orders[1])) == N
    sc.close()


def test_abandoned_iteration_is_stopped_before_the_next_one(data, workers):
    dls = _loaders(data, device_image_stream=True)
    dl = dls["train"]
    dl.sampler.set_epoch(0)
    torch.manual_seed(100)
    abandoned = iter(dl)
    first = next(abandoned)
    got = _run(dls)   # a complete pass over both splits on the same staging
    _assert_same(got, workers())
    assert torch.equal(first[0].cpu(), got["train"][0][0][0]) and torch.equal(first[1].cpu(), got["train"][0][0][1])
    with pytest.raises(RuntimeError, match="abandoned"):
        for _ in abandoned:
            pass
    _close(dls)


# ---- child processes ---------------------------------------------------------------------------------------------------------------------
def _env():
    return dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")


def _same(a, b) -> bool:
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b)


def test_console_test_with_the_stream(data, tmp_path):
    """`yogo test CKPT DEFN --dump-to-disk` over the 23 files as a test split: the same line, an equal pickled tuple"""
    from yogo_amd.model import YOGO

    torch.manual_seed(3)
    net = YOGO(HW, 0.0425, 0.0555, 4).cuda()
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
    lines, dumps = [], []
    for extra in ([], ["--device-image-stream"]):
        cwd = tmp_path / ("stream" if extra else "workers")
        cwd.mkdir()
        r = subprocess.run([sys.executable, "-m", "yogo_amd", "test", str(pth), str(data[3]["test"]), "--dump-to-disk", *extra], cwd=cwd,
                           env=_env(), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines.append([ln for ln in r.stdout.splitlines() if "test loss" in ln])
        assert ("device image stream (test): 23 images in 1 groups, 6 decoded on the host" in r.stdout) is bool(extra), r.stdout
        with open(cwd / "test_metrics.pkl", "rb") as f:
            dumps.append(pickle.load(f))
    assert lines[0] and lines[0] == lines[1], lines
    assert isinstance(dumps[0], tuple) and _same(dumps[0], dumps[1])


def test_train_with_the_stream_in_a_child_process(data, tmp_path):
    """`train DEFN --device-image-stream -bs 4 --epochs 1 --image-hw 70 37` finishes and logs what the stream of each split did
    (at the default decode group of 1 024 images every split is one group)"""
    r = subprocess.run([sys.executable, "-m", "yogo_amd", "train", str(data[3]["plain"]), "--device-image-stream", "-bs", "4", "--epochs", "1",
                        "--image-hw", str(HW[0]), str(HW[1]), "--name", "stream_cli"], cwd=tmp_path, env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device image stream (train): 17 images in 1 groups" in r.stdout and "device image stream (val): 6 images in 1 groups" in r.stdout
    assert "device image cache" not in r.stdout and (tmp_path / "trained_models" / "stream_cli" / "best.pth").exists()
