"""Decoded images resident in HBM (yogo_amd/image_cache.py, yogo_amd/csrc/image_cache.hip) on the MI355X: the gather bit for
bit against a torch restatement (uint8 and fp32 / 255), the cached loader's batches equal to the uncached loader's over three
epochs (full and partial residency, normalize_images, rgb, resized files, an unreadable file, thumbnail augmentation, spawn
workers), no worker pool for a fully resident split, `train` end to end with and without the cache, and two ranks on one card."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from _image_cache_data import write_defn, write_images

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
DEV = torch.device("cuda", 0)
Sx, Sy = 12, 8


# ---- the gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,S,B", [((1, 772, 1032), 160, 128), ((3, 50, 70), 9, 12), ((3, 64, 96), 7, 10)])
@pytest.mark.parametrize("fp32", [False, True])
def test_gather_bit_exact(shape, S, B, fp32):
    from yogo_amd.image_cache import gather

    g = torch.Generator().manual_seed(S * 31 + B)
    cache_cpu = torch.randint(0, 256, (S, *shape), dtype=torch.uint8, generator=g)
    cache_cpu[0].view(-1)[:256] = torch.arange(256, dtype=torch.uint8)   # every byte value at least once
    cache = cache_cpu.to(DEV)
    slots = torch.randint(0, S, (B,), generator=g)
    slots[1] = slots[0]                                                   # repeated slots
    slots[2], slots[5], slots[B - 1] = 0, -1, -1                          # rows left alone
    slots[3] = S - 1
    sentinel = -1.5 if fp32 else 77
    out = torch.full((B, *shape), sentinel, dtype=torch.float32 if fp32 else torch.uint8, device=DEV)
    gather(cache, slots, out)
    torch.cuda.synchronize()
    for b in range(B):
        s = int(slots[b])
        got = out[b].cpu()
        if s < 0:
            assert bool((got == sentinel).all()), b
        else:
            want = cache_cpu[s] / 255 if fp32 else cache_cpu[s]
            assert got.dtype == want.dtype and torch.equal(got, want), (b, s)
    # the checks before the launch
    with pytest.raises(IndexError):
        gather(cache, [S] + [0] * (B - 1), out)
    with pytest.raises(ValueError):
        gather(cache, [0] * (B - 1), out)
    with pytest.raises(ValueError):
        gather(cache, [0] * B, out.to(torch.float16))
    with pytest.raises(ValueError):
        gather(cache.float(), [0] * B, out)
    with pytest.raises(ValueError):
        gather(cache, [0], out[:, :, :1])                                 # wrong shape
    nc = torch.empty(B, shape[0], shape[2], shape[1], dtype=out.dtype, device=DEV).transpose(2, 3)   # the right shape, not contiguous
    with pytest.raises(ValueError):
        gather(cache, [0] * B, nc)
    with pytest.raises(RuntimeError, match="MI355X"):
        gather(cache_cpu, [0] * B, out)


# ---- the loader ------------------------------------------------------------------------------------------------------------
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


def _epochs(dls, epochs: int = 3):
    """{split: [epoch][batch] (imgs, labels) on the host} with torch.manual_seed(e) before epoch e"""
    out = {}
    for name in ("train", "val"):
        dl, res = dls[name], []
        for e in range(epochs):
            dl.sampler.set_epoch(e)
            torch.manual_seed(e)
            res.append([(i.cpu(), l.cpu()) for i, l in dl])
        out[name] = res
    return out


def _assert_same(got, want):
    for name in ("train", "val"):
        assert len(got[name]) == len(want[name])
        for e, (ge, we) in enumerate(zip(got[name], want[name])):
            assert len(ge) == len(we), (name, e)
            for k, ((gi, gl), (wi, wl)) in enumerate(zip(ge, we)):
                assert gi.dtype == wi.dtype and torch.equal(gi, wi), (name, e, k)
                assert torch.equal(gl, wl), (name, e, k)


VARIANTS = {
    "plain": {},
    "normalize": {"normalize_images": True},
    "rgb": {"rgb": True},
    "resize": {"file_hw": (100, 130), "image_hw": (96, 128)},
    "truncated": {"truncated": [5]},
    "thumbnails": {"thumbnails": True},
}


def _loaders(tmp_path: Path, variant: str, residency: str, n: int = 24, bs: int = 4):
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.yogo_dataloader import get_dataloader

    v = VARIANTS[variant]
    image_hw = v.get("image_hw", (64, 96))
    img_dir, lab_dir = write_images(tmp_path / "data", n, hw=v.get("file_hw", image_hw), rgb=v.get("rgb", False), seed=3,
                                    truncated=v.get("truncated", ()))
    defn = DatasetDefinition.from_yaml(write_defn(tmp_path, img_dir, lab_dir, _thumbs(tmp_path / "thumbs") if v.get("thumbnails") else None))
    per = (3 if v.get("rgb") else 1) * image_hw[0] * image_hw[1]
    n_train = int(0.75 * n)
    gib = 1.0 if residency == "full" else round(0.4 * n_train) * per / 2 ** 30
    kw = dict(Sx=Sx, Sy=Sy, training=True, image_hw=image_hw, rgb=v.get("rgb", False), normalize_images=v.get("normalize_images", False),
              device=DEV)
    return (get_dataloader(defn, bs, device_image_cache_gib=gib, **kw), get_dataloader(defn, bs, **kw))


@pytest.mark.parametrize("residency", ["full", "partial"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_loader_identity(tmp_path, variant, residency):
    cached, plain = _loaders(tmp_path, variant, residency)
    assert cached["train"].cache is not None and plain["train"].cache is None
    tc = cached["train"].cache
    if residency == "full":
        assert tc.S == 18 and cached["val"].cache is not None and cached["val"].cache.S == 6
    else:
        assert tc.S == 7 and cached["val"].cache is None   # about 40 % of the train split; nothing left for val
    got, want = _epochs(cached), _epochs(plain)
    _assert_same(got, want)
    assert tc.full == (residency == "full" and variant not in ("truncated", "thumbnails"))
    if variant == "truncated":   # the unreadable file is not resident (it stays with the loader, which drops it every epoch)
        unreadable = sum(_split_file(cached["train"].dataset, i) == 5 for i in range(tc.S))
        assert int(tc.resident.sum()) == tc.S - unreadable
    assert len(cached["train"]) == len(plain["train"]) and cached["train"].batch_size == plain["train"].batch_size
    assert type(cached["train"].dataset) is type(plain["train"].dataset) and len(cached["train"].dataset) == len(plain["train"].dataset)


def _split_file(split, i):
    from yogo_amd.image_cache import resolve_sample

    ds, j = resolve_sample(split, i)
    return int(Path(str(ds._image_paths[j])).stem.split("_")[1])


def test_loader_identity_with_spawn_workers(tmp_path, monkeypatch):
    """partial residency with two spawn workers per split: the prefill's one-off pool and the persistent pool of the split, which
    receives the pickled ResidentMarkers after the prefill"""
    import yogo_amd.yogo_dataloader as ydl

    monkeypatch.setattr(ydl, "choose_dataloader_num_workers", lambda n, requested=None: 2)
    cached, plain = _loaders(tmp_path, "truncated", "partial")
    assert cached["train"].loader.num_workers == 2 and cached["train"].cache.num_workers == 2
    _assert_same(_epochs(cached, 2), _epochs(plain, 2))


class _NoIter:
    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        raise AssertionError("the host DataLoader of a fully resident split was iterated")


def test_fully_resident_split_needs_no_workers(tmp_path, monkeypatch):
    import yogo_amd.yogo_dataloader as ydl
    from yogo_amd import _hip

    monkeypatch.setattr(ydl, "choose_dataloader_num_workers", lambda n, requested=None: 2)
    cached, plain = _loaders(tmp_path, "plain", "full")
    want = _epochs(plain, 2)
    for name in ("train", "val"):
        dl = cached[name]
        dl.cache.prefill()   # the one-off pool of the prefill (2 spawn workers), then the split's own loader is never iterated
        assert dl.cache.full
        dl.loader = _NoIter(dl.loader)
    _hip.launch_log(True)
    got = _epochs(cached, 2)
    log = _hip.read_launch_log()
    _hip.launch_log(False)
    _assert_same(got, want)
    gathers = [ln for ln in log if ln.startswith("image_cache_gather_vec_kernel<u8>")]
    assert len(gathers) == 2 * (len(cached["train"]) + len(cached["val"]))
    for name in ("train", "val"):
        assert cached[name].loader.loader._iterator is None   # no persistent worker pool was ever started


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _flat(obj):
    if isinstance(obj, torch.Tensor):
        return [obj.detach().cpu()]
    if isinstance(obj, dict):
        return [t for k in sorted(obj, key=str) for t in _flat(obj[k])]
    if isinstance(obj, (list, tuple)):
        return [t for v in obj for t in _flat(v)]
    return [torch.tensor(float(obj))] if isinstance(obj, (int, float)) else []


def test_train_end_to_end_with_and_without_cache(tmp_path):
    from yogo_amd.trainer import Trainer, build_config
    from yogo_amd.utils.argparsers import global_parser

    img_dir, lab_dir = write_images(tmp_path / "data", 24, hw=(64, 96), seed=5)
    defn = write_defn(tmp_path, img_dir, lab_dir)
    runs = {}
    for tag, extra in (("cached", ["--device-image-cache", "1"]), ("plain", [])):
        args = global_parser().parse_args(["train", str(defn), "--epochs", "3", "-bs", "4", "--image-hw", "64", "96", "--half",
                                           "--name", "cache_e2e", *extra])
        config = build_config(args)
        config["trained_models_dir"] = str(tmp_path / tag)
        torch.manual_seed(0)
        trainer = Trainer.train_from_ddp(0, 1, config)
        assert (trainer.train_dataloader.cache is not None) == (tag == "cached")
        ckpt = torch.load(tmp_path / tag / "cache_e2e" / "best.pth", map_location="cpu", weights_only=False)
        runs[tag] = (ckpt["model_state_dict"], _flat(trainer.backend.optimizer_state_dict()), trainer.global_step)
    (sd_c, opt_c, steps_c), (sd_p, opt_p, steps_p) = runs["cached"], runs["plain"]
    assert steps_c == steps_p == 3 * 5
    assert sd_c.keys() == sd_p.keys()
    for k in sd_p:
        assert torch.equal(sd_c[k], sd_p[k]), k
    # the optimiser state after the third epoch (the checkpoint holds the weights of the epoch-0 validation)
    assert len(opt_c) == len(opt_p) > 0 and all(torch.equal(a, b) for a, b in zip(opt_c, opt_p))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_on_one_card(tmp_path):
    img_dir, lab_dir = write_images(tmp_path / "data", 40, hw=(64, 96), seed=9, truncated=[7])
    defn = write_defn(tmp_path, img_dir, lab_dir)
    world, port = 2, str(_free_port())
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(HERE / "image_cache_dp_worker.py"), str(r), str(world), port, str(tmp_path), str(defn)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    res = [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(world)]
    for r in range(world):   # each rank keeps every index of train and val, but the truncated file's
        assert res[r]["batches"] > 0 and res[r]["resident"] == res[r]["S"] - 1 and res[r]["S"] == 40
    assert res[0]["order"] != res[1]["order"]   # the ranks saw different indices
