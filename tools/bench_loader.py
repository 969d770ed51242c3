"""Training data through the loader, with and without the device image cache (yogo_amd/image_cache.py), on one MI355X.

Writes ~1024 synthetic 772 x 1032 gray PNGs with label files into a temporary directory (16 encoder processes; deleted at the
end): a smooth background plus Gaussian noise of sigma 6, which PIL's default zlib level compresses to about 65 % -- decode
time depends on content, so these numbers stand for images like that, not for every dataset.  The worker pool is pinned at 16
(choose_dataloader_num_workers is wrapped in-process; left alone it sizes the pool from the host's full core count).
Reports: uncached loader images/s, prefill images/s, resident loader images/s, HipTrainer(half=True) ms/step at B = 128 fed by
each loader against device-generated batches in the same process (device events, warmed up), the HBM bytes the cache holds,
and, with event timing, one uploaded batch, one flip pass and one gather.

  python tools/bench_loader.py [--images 1024] [--epochs 2]
  python tools/bench_loader.py --gather-only        (the gather, flip and upload alone: run it under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, B, WORKERS = 772, 1032, 128, 16


def _encode(args):
    k, out = args
    from PIL import Image

    rng = np.random.default_rng(k)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    a, b, c = rng.uniform(0.5, 2.0, 3)
    smooth = 150 + 40 * np.sin(x / W * np.pi * a + c) * np.cos(y / H * np.pi * b)
    img = np.clip(smooth + rng.normal(0, 6, size=(H, W)), 0, 255).astype(np.uint8)
    Image.fromarray(img, mode="L").save(os.path.join(out, "images", f"img_{k:05d}.png"))
    rows = [f"{int(rng.integers(0, 4))} {rng.uniform(0.05, 0.95):.6f} {rng.uniform(0.05, 0.95):.6f} 0.040000 0.050000" for _ in range(20)]
    with open(os.path.join(out, "labels", f"img_{k:05d}.txt"), "w") as f:
        f.write("\n".join(rows) + "\n")


def write_dataset(root: str, n: int) -> str:
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "labels"))
    with ProcessPoolExecutor(WORKERS) as ex:
        list(ex.map(_encode, [(k, root) for k in range(n)], chunksize=8))
    defn = os.path.join(root, "defn.yml")
    with open(defn, "w") as f:
        f.write("class_names: [you, only, glance, once]\ndataset_split_fractions: {train: 1.0, val: 0.0}\n"
                f"dataset_paths:\n  a: {{image_path: {root}/images, label_path: {root}/labels}}\n")
    return defn


def time_loader(dl, epochs: int):
    """images/s over `epochs` epochs (after one warm-up epoch that starts the workers)"""
    for _ in dl:
        pass
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    for e in range(epochs):
        dl.sampler.set_epoch(e + 1)
        for imgs, _ in dl:
            n += imgs.shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def time_steps(tr, batches, dev):
    """ms per step over the iterable `batches` ((imgs, labels) pairs), device events around the whole loop"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    n = 0
    for imgs, labels in batches:
        tr.step(imgs, labels)
        n += 1
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / max(n, 1), n


def event_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels_alone(dev, reps=50):
    from yogo_amd.data import flip_batch
    from yogo_amd.image_cache import gather

    g = torch.Generator().manual_seed(0)
    cache = torch.randint(0, 256, (160, 1, H, W), dtype=torch.uint8, generator=g).to(dev)
    slots = torch.randint(0, 160, (B,), generator=g)
    out8 = torch.empty(B, 1, H, W, dtype=torch.uint8, device=dev)
    out32 = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
    lab = torch.zeros(B, 6, 97, 129, device=dev)
    pinned = torch.empty(B, 1, H, W, dtype=torch.uint8).pin_memory()
    pageable = torch.empty(B, 1, H, W, dtype=torch.uint8)
    per = H * W
    res = {}
    res["gather_u8_ms"] = event_ms(lambda: gather(cache, slots, out8), reps)
    res["gather_f32_ms"] = event_ms(lambda: gather(cache, slots, out32), reps)
    res["gather_u8_TBps"] = 2 * B * per / res["gather_u8_ms"] / 1e9
    res["gather_f32_TBps"] = 5 * B * per / res["gather_f32_ms"] / 1e9
    res["flip_u8_ms"] = event_ms(lambda: flip_batch(out8, lab, True, True), reps)
    res["flip_f32_ms"] = event_ms(lambda: flip_batch(out32, lab, True, True), reps)
    res["upload_pinned_u8_ms"] = event_ms(lambda: pinned.to(dev, non_blocking=True), 10)
    res["upload_pageable_u8_ms"] = event_ms(lambda: pageable.to(dev, non_blocking=True), 10)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--gather-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loader needs the MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.gather_only:
        print(json.dumps(kernels_alone(dev)), flush=True)
        return

    import yogo_amd.yogo_dataloader as ydl
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.model import YOGO
    from yogo_amd.synthetic import synthetic_images, synthetic_labels
    from yogo_amd.train import HipTrainer
    from yogo_amd.yogo_loss import YOGOLoss

    ydl.choose_dataloader_num_workers = lambda n, requested=None: WORKERS
    root = tempfile.mkdtemp(prefix="yogo_loader_bench_")
    try:
        t0 = time.perf_counter()
        defn = DatasetDefinition.from_yaml(write_dataset(os.path.join(root, "d"), args.images))
        png = sum(os.path.getsize(os.path.join(root, "d", "images", f)) for f in os.listdir(os.path.join(root, "d", "images")))
        print(f"[bench_loader] wrote {args.images} PNGs in {time.perf_counter() - t0:.1f} s, {png / (args.images * H * W):.1%} of raw",
              flush=True)
        torch.manual_seed(0)
        model = YOGO((H, W), 0.0425, 0.0555, 4).to(dev)
        model.train()
        tr = HipTrainer(model, YOGOLoss().to(dev), total_steps=10 ** 6, half=True)
        kw = dict(Sx=model.Sx, Sy=model.Sy, training=True, image_hw=(H, W), device=dev)
        res = {"images": args.images, "workers": WORKERS, "batch": B, "png_bytes_over_raw": png / (args.images * H * W)}

        plain = ydl.get_dataloader(defn, B, **kw)["train"]
        res["uncached_loader_img_per_s"] = time_loader(plain, args.epochs)
        cached = ydl.get_dataloader(defn, B, device_image_cache_gib=args.images * H * W / 2 ** 30 + 0.01, **kw)["train"]
        cache = cached.cache
        t0 = time.perf_counter()
        cache.prefill()
        res["prefill_img_per_s"] = int(cache.resident.sum()) / (time.perf_counter() - t0)
        res["cache_hbm_bytes"] = cache.nbytes
        res["cache_full"] = cache.full
        res["resident_loader_img_per_s"] = time_loader(cached, args.epochs)

        imgs = synthetic_images(B, H, W, device=dev, seed=100)
        labels = synthetic_labels(B, model.Sx, model.Sy, K=64, num_classes=4, device=dev, seed=200)
        steps = max(8, args.epochs * len(cached))
        time_steps(tr, [(imgs, labels)] * 10, dev)   # warm-up
        for rep in range(2):   # alternate the three feeds, twice
            res[f"step_ms_device_batches_{rep}"], _ = time_steps(tr, [(imgs, labels)] * steps, dev)
            res[f"step_ms_resident_loader_{rep}"], _ = time_steps(tr, (b for e in range(args.epochs) for b in cached), dev)
            res[f"step_ms_uncached_loader_{rep}"], _ = time_steps(tr, (b for e in range(args.epochs) for b in plain), dev)
        res.update(kernels_alone(dev))
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
