"""Thumbnail ("blob") augmentation on the MI355X (yogo_amd/csrc/blobgen.hip): bit-exact against the numpy restatement of
tests/_blobgen_ref.py (images, label rows, counts, label tensors; uint8 and normalize_images), the crowded case that reaches
the second chunk of tries and the skip path, the reference's invariants without the hash, determinism, the device loader
with mixed / all-synthetic batches and flips, and `yogo train` end to end on a definition with thumbnails."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import _blobgen_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DATA = ROOT / "tests" / "fake-data" / "data"
CLASSES = ["you", "only", "glance", "once"]
DEV = torch.device("cuda", 0)


def _write_thumbs(root: Path, per_class: dict, seed: int) -> dict:
    """{class name: [dir]} with random thumbnails; per_class: {name: [(h, w), ...]}"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, dims in per_class.items():
        d = root / name
        d.mkdir(parents=True, exist_ok=True)
        for k, (h, w) in enumerate(dims):
            base = int(rng.integers(150, 256))
            arr = np.clip(rng.normal(base, 40, size=(h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(arr, mode="L").save(d / f"t{k:04d}.png")
        out[name] = [d]
    return out


def _dims(rng, count, lo, hi):
    return [(int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for _ in range(count)]


@pytest.fixture(scope="module")
def production(tmp_path_factory):
    from yogo_amd.blobgen import BlobDataset

    rng = np.random.default_rng(0)
    dirs = _write_thumbs(tmp_path_factory.mktemp("prod"), {c: _dims(rng, 100, 23, 80) for c in ("you", "glance", "once")}, 1)
    return BlobDataset(dirs, 129, 97, CLASSES, n=100, length=4000, seed=11)


@pytest.fixture(scope="module")
def crowded(tmp_path_factory):
    from yogo_amd.blobgen import BlobDataset

    rng = np.random.default_rng(2)
    per = {"only": _dims(rng, 20, 30, 60), "once": _dims(rng, 20, 30, 60) + [(119, 30)]}
    dirs = _write_thumbs(tmp_path_factory.mktemp("crowd"), per, 3)
    return BlobDataset(dirs, 20, 15, CLASSES, n=100, length=100, background_img_shape=(120, 160), seed=5)


def _ref_labels(rows, counts, Sx, Sy):
    from yogo_amd.data import format_labels_batch

    return format_labels_batch([torch.from_numpy(rows[s, :counts[s]].copy()) for s in range(len(counts))], Sx, Sy, "xyxy", device=DEV)


def _check_exact(bd, indices, epoch):
    H, W = bd.background_img_shape
    want_imgs, want_rows, want_counts, placed = R.generate(bd.atlas.numpy(), bd.table.numpy(), indices, bd.seed, epoch, bd.n, H, W)
    imgs, labels, rows, counts = bd.generate(indices, epoch)
    torch.cuda.synchronize()
    assert torch.equal(counts.cpu(), torch.from_numpy(want_counts))
    assert torch.equal(rows.cpu(), torch.from_numpy(want_rows))
    assert torch.equal(imgs.cpu()[:, 0], torch.from_numpy(want_imgs))
    assert torch.equal(labels, _ref_labels(want_rows, want_counts, bd.Sx, bd.Sy))
    _, _, _, background = bd.place(indices, epoch)
    assert background.cpu().tolist() == [p["background"] for p in placed]
    return placed


def test_bit_exact_against_restatement_production_shape(production):
    idx = list(range(100, 116))
    _check_exact(production, idx, 3)
    # normalize_images: the same images / 255 in fp32, correctly rounded
    production.normalize_images = True
    try:
        imgs, _, _, _ = production.generate(idx, 3)
    finally:
        production.normalize_images = False
    want, _, _, _ = production.generate(idx, 3)
    assert imgs.dtype == torch.float32 and torch.equal(imgs.cpu(), want.cpu().float() / 255)


def test_crowded_reaches_second_chunk_and_skip(crowded):
    placed = _check_exact(crowded, list(range(16)), 0)
    assert sum(p["exhausted"] for p in placed) > 0, "no slot exhausted its 100 tries"
    assert max(t for p in placed for t in p["accepted_tries"]) >= 64, "no slot accepted a try of the second chunk"
    # the H - 1 tall thumbnail can only go to y = 0
    tall = int(np.nonzero(crowded.table[:, 1].numpy() == 119)[0][0])
    ys = [y for p in placed for (t, x, y, fl) in p["boxes"] if t == tall]
    assert ys and all(y == 0 for y in ys)


def test_reference_invariants(production):
    bd = production
    H, W = bd.background_img_shape
    idx = list(range(32))
    imgs, _, rows, counts = bd.generate(idx, 1)
    boxes, rows2, counts2, background = bd.place(idx, 1)
    assert torch.equal(rows2, rows) and torch.equal(counts2, counts)
    imgs, boxes, rows, counts, background = imgs.cpu()[:, 0], boxes.cpu(), rows.cpu(), counts.cpu(), background.cpu()
    table, atlas = bd.table, bd.atlas
    flips = []
    for s in range(len(idx)):
        c = int(counts[s])
        assert 0 < c <= bd.n
        covered = torch.zeros(H, W, dtype=torch.bool)
        bx = []
        for k in range(c):
            t, x, y, fl = boxes[s, k].tolist()
            off, h, w, cls, _ = table[t].tolist()
            assert 0 <= x and x + w < W and 0 <= y and y + h < H
            th = atlas[off:off + h * w].reshape(h, w)
            if fl & 1:
                th = th.flip(1)
            if fl & 2:
                th = th.flip(0)
            assert torch.equal(imgs[s, y:y + h, x:x + w], th)
            assert not covered[y:y + h, x:x + w].any(), "boxes intersect"
            covered[y:y + h, x:x + w] = True
            assert float(rows[s, k, 0]) == cls
            bx.append((x, y, x + w, y + h))
            flips.append(fl)
        assert (imgs[s][~covered] == int(background[s])).all()
        if c == bd.n:   # every draw placed: the background is the truncated mean of their shades
            shades = [int(table[int(boxes[s, k, 0]), 4]) for k in range(c)]
            assert int(background[s]) == int(np.float32(np.mean(shades)))
    fl = np.array(flips)
    N = len(fl)
    assert N >= 2000
    for bit in (1, 2):
        rate = float(((fl & bit) > 0).mean())
        assert abs(rate - 0.5) < 4 * np.sqrt(0.25 / N), (bit, rate)


def test_determinism(production):
    bd = production
    batch = list(range(200, 232))
    imgs, labels, rows, counts = bd.generate(batch, 2)
    for j in (0, 7, 31):
        one = bd.generate([batch[j]], 2)
        assert torch.equal(one[0][0], imgs[j]) and torch.equal(one[1][0], labels[j])
        assert torch.equal(one[2][0], rows[j]) and torch.equal(one[3][0], counts[j])
    other = bd.generate(batch, 3)[0]
    assert not torch.equal(other, imgs)
    # written into given rows of a caller's batch: the other rows stay untouched
    out = torch.full((40, 1) + bd.background_img_shape, 7, dtype=torch.uint8, device=DEV)
    pos = [39, 0, 5]
    got, _, _, _ = bd.generate([batch[0], batch[1], batch[2]], 2, out_imgs=out, positions=pos)
    assert got is out
    for j, p in enumerate(pos):
        assert torch.equal(out[p], imgs[j])
    assert int((out[1:5] != 7).sum()) == 0


def _thumb_defn(tmp_path: Path, dims) -> Path:
    dirs = _write_thumbs(tmp_path / "thumbs", {"glance": dims, "once": dims[::-1]}, 7)
    defn = tmp_path / "defn.yml"
    defn.write_text(
        "class_names: [you, only, glance, once]\n"
        "dataset_split_fractions: {train: 0.75, val: 0.25}\n"
        f"dataset_paths:\n  a: {{image_path: {DATA}/images1, label_path: {DATA}/labels1}}\n  b: {{image_path: {DATA}/images2, label_path: {DATA}/labels2}}\n"
        f"  c: {{image_path: {DATA}/images3, label_path: {DATA}/labels3}}\n"
        f"thumbnail_augmentation:\n  glance: {dirs['glance'][0]}\n  once: {dirs['once'][0]}\n")
    return defn


def test_device_loader_mixed_batches(tmp_path):
    from yogo_amd.data import flip_batch, format_labels_batch
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.yogo_dataloader import collate_mixed, get_dataloader

    defn = DatasetDefinition.from_yaml(_thumb_defn(tmp_path, [(24, 24), (25, 30), (22, 28), (26, 26)]))
    Sx, Sy, hw, bs = 12, 8, (64, 96), 3
    dl = get_dataloader(defn, bs, Sx, Sy, training=False, image_hw=hw)["train"]
    real, blob = dl.dataset.datasets
    L = len(real)
    assert len(blob) == L // 2 and len(dl.dataset) == L + L // 2
    dl.sampler.set_epoch(1)
    order = list(iter(dl.sampler))
    batches = list(dl)
    assert sum(int(imgs.shape[0]) for imgs, _ in batches) == L + L // 2
    for k, (imgs, labels) in enumerate(batches):
        assert imgs.dtype == torch.uint8 and tuple(imgs.shape[1:]) == (1,) + hw
        for j, i in enumerate(order[k * bs:(k + 1) * bs]):
            if i >= L:
                want_img, want_lab, _, _ = blob.generate([i - L], 1)
                assert torch.equal(imgs[j], want_img[0]) and torch.equal(labels[j], want_lab[0])
            else:
                img, rows = real[i]
                assert torch.equal(imgs[j].cpu(), img)
                assert torch.equal(labels[j], format_labels_batch([rows], Sx, Sy, "cxcywh", device=DEV)[0])
    # a batch made only of synthetic items
    imgs, labels = dl._assemble(collate_mixed([1, 0]), DEV)
    want_img, want_lab, _, _ = blob.generate([1, 0], 1)
    assert torch.equal(imgs, want_img) and torch.equal(labels, want_lab)

    # training: the batch flips cover the synthetic rows too (the same host draws, in the same order)
    seed = next(s for s in range(100) if _both_flip(s))
    tl = get_dataloader(defn, bs, Sx, Sy, training=True, image_hw=hw)["train"]
    tl.sampler.set_epoch(1)
    torch.manual_seed(seed)
    flipped = list(tl)
    assert len(flipped) == len(batches)
    torch.manual_seed(seed)
    for (imgs, labels), (fi, fl) in zip(batches, flipped):
        h, v = bool(torch.rand(1) < 0.5), bool(torch.rand(1) < 0.5)
        wi, wl = flip_batch(imgs, labels, h, v)
        assert torch.equal(fi, wi) and torch.equal(fl, wl)


def _both_flip(seed: int) -> bool:
    g = torch.random.get_rng_state()
    torch.manual_seed(seed)
    both = bool(torch.rand(1) < 0.5) and bool(torch.rand(1) < 0.5)
    torch.random.set_rng_state(g)
    return both


def test_train_cli_with_thumbnails(tmp_path):
    defn = _thumb_defn(tmp_path, [(24, 24), (30, 40), (26, 28), (40, 30)])
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "yogo_amd", "train", str(defn), "--epochs", "1", "-bs", "4", "--image-hw", "128", "192",
                        "--half", "--name", "blobs"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "trained_models" / "blobs" / "best.pth").exists()
