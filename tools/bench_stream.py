"""Labelled batches on one MI355X: the device image stream (`--device-image-stream`: yogo_amd/image_stream.py on png_prefill.Filler,
csrc/inflate.hip, csrc/png_unpack_planes.hip, csrc/image_cache.hip) against the DataLoader's PIL workers, in the same process on the
same machine.

Input: --frames seeded 772 x 1032 8-bit grey frames written as PNG by PIL with two label rows each, in the two contents of
tools/bench_png_feed.py (`noise`, `smooth`), as tools/bench_prefill.py writes them, into a temporary directory that is removed at the
end; the files are read back once before anything is timed (reads come from the page cache).  Per content one child process with its
own time limit runs every leg; a leg is the four passes  workers, stream, stream, workers  in that order, each over all frames once
with loaders of its own (the worker route: CPUS persistent spawn workers, started inside the clock as in a run's first epoch; the
stream: CPUS reader threads, its staging and scratch allocated inside the clock too):

  feed     the loader alone at training=False, batch 64; the consumer sums every batch's pixels on the device
  test     ``Trainer.test`` with device metrics (what `yogo test --device-metrics` runs) at batch 64, bf16, untrained weights
  train    the train-side loader (shuffled, both flips) at batch 128 without a cache, TWO epochs per loader -- in the second the
           workers are up and the stream's buffers are there, as in every later epoch of a run; the consumer as in `feed` (no
           training step)
  sweep    `feed` on the stream alone at stream_decode_batch 256 / 1024 / 2048

Per pass: images/s = frames / seconds on the host clock from ``iter()`` to the final device synchronise, the seconds until the first
batch was on the device, and for the stream its groups, what the host decoded, its HBM bytes (two staging tensors + scratch) and its
pinned bytes.  The passes of a leg must sum the same pixels.  The lines are APPENDED to --out.

  python tools/bench_stream.py [--frames 2048] [--content noise,smooth] [--legs feed,test,train,sweep] [--out profiles/image_stream.log]
"""
import argparse
import gc
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_png_feed import CLASSES, H, W, _spans, _write   # noqa: E402  (the frame sets of the inference feed's benchmark)

CPUS = 16
DECODE_BATCHES = (256, 1024, 2048)
DEFAULT_BATCH = 1024   # yogo_amd.png_prefill.DEFAULT_DECODE_BATCH
Sx, Sy = 129, 97       # the grid of the model at 772 x 1032


class Timed:
    """a loader that notes when its first batch was on the device"""

    def __init__(self, dl):
        self.dl, self.first, self.t0 = dl, None, None

    def __getattr__(self, name):
        return getattr(self.dl, name)

    def __len__(self):
        return len(self.dl)

    def __iter__(self):
        import torch

        self.t0 = time.perf_counter()
        for item in self.dl:
            if self.first is None:
                torch.cuda.synchronize()
                self.first = time.perf_counter() - self.t0
            yield item


def _loader(split, batch_size: int, training: bool, stream: bool, decode_batch: int = DEFAULT_BATCH):
    import yogo_amd.yogo_dataloader as ydl
    from yogo_amd.data import RandomHorizontalFlipWithBBs, RandomVerticalFlipWithBBs
    from yogo_amd.image_stream import Scratch

    ydl.choose_dataloader_num_workers = lambda n, requested=None: CPUS   # a single rank's share of this machine's CPUs
    augs = [RandomHorizontalFlipWithBBs(0.5), RandomVerticalFlipWithBBs(0.5)] if training else []
    sc = Scratch((1, H, W), batch_size, decode_batch, "cuda", max_threads=CPUS) if stream else None
    return Timed(ydl._get_dataloader(split, batch_size, augs, 0, 1, Sx, Sy, "cuda", strict_steps=training, image_shape=(1, H, W),
                                     name="bench", scratch=sc))


def _done(dl) -> dict:
    """what the pass's stream reports, and everything it holds released (the worker route: its persistent workers shut down)"""
    res = {}
    if dl.stream is not None:
        s = dl.stream.stats
        res = {k: s[k] for k in ("groups", "streamed", "host_decoded", "hbm_bytes", "pinned_bytes")}
        dl.stream.scratch.close()
    it = getattr(dl.loader, "_iterator", None)
    if it is not None:
        it._shutdown_workers()
        dl.loader._iterator = None
    return res


def _pass(log, what: str, dl, consume, epochs: int = 1) -> int:
    """`epochs` passes over one loader (from the second on its workers are up and the stream's staging and scratch are there)"""
    import torch

    n = len(dl.dataset)
    times = []
    for e in range(epochs):
        dl.sampler.set_epoch(e)
        dl.first = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        checksum = consume(dl)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0, dl.first))
    st = _done(dl)
    extra = ""
    if st:
        extra = (f"; {st['groups']} groups, {st['host_decoded']} of {st['streamed']} decoded on the host, {st['hbm_bytes'] / 2 ** 30:.2f} GiB HBM + "
                 f"{st['pinned_bytes'] / 2 ** 30:.2f} GiB pinned")
    for e, (dt, first) in enumerate(times):
        log(f"  {what if e == 0 else '  ... its epoch ' + str(e + 1):<28s} {dt:7.2f} s = {n / dt:7.0f} img/s   first batch after {first:6.2f} s"
            f"{extra if e == epochs - 1 else ''}; checksum {checksum}")
    del dl
    gc.collect()
    return checksum


def step(d: str, out: str, which: str) -> int:
    import torch

    from yogo_amd.model import YOGO
    from yogo_amd.trainer import Trainer
    from yogo_amd.yogo_dataset import ObjectDetectionDataset

    def log(s=""):
        print(s, flush=True)
        with open(out, "a") as f:
            f.write(s + "\n")

    split = ObjectDetectionDataset(os.path.join(d, "images"), os.path.join(d, "labels"), Sx, Sy, CLASSES, image_hw=(H, W))
    torch.zeros(1, device="cuda")   # the device is up before the clock starts, as in a run

    def pixels(dl) -> int:
        acc = torch.zeros((), dtype=torch.int64, device="cuda")
        for imgs, labels in dl:
            acc += imgs.sum(dtype=torch.int64) + labels.shape[0]
        return int(acc)

    torch.manual_seed(0)
    net = YOGO((H, W), 0.0425, 0.0555, len(CLASSES)).cuda()
    assert tuple(net.get_grid_size()) == (Sx, Sy), net.get_grid_size()
    config = {"class_names": CLASSES, "no_obj_weight": 0.5, "iou_weight": 1, "label_smoothing": 0.0001, "half": True}

    def test(dl) -> int:
        res = Trainer.test(dl, "cuda", config, net, include_mAP=False, device_metrics=True)
        return int(res[10])   # the number of true objects the metrics saw

    legs = (("feed", 64, False, pixels, 1), ("test", 64, False, test, 1), ("train", 128, True, pixels, 2))
    for name, bs, training, consume, epochs in legs:
        if name not in which.split(","):
            continue
        log(f" leg {name}: batch {bs}" + (f", {epochs} epochs per loader" if epochs > 1 else ""))
        sums = {_pass(log, f"{route} ({CPUS} {'threads' if stream else 'workers'})", _loader(split, bs, training, stream), consume, epochs)
                for route, stream in (("workers", False), ("stream", True), ("stream", True), ("workers", False))}
        log(f"  all four passes saw the same: {len(sums) == 1}")
        if len(sums) != 1:
            return 1
    if "sweep" not in which.split(","):
        return 0
    log(" leg sweep: feed at batch 64, the stream alone")
    for db in DECODE_BATCHES:
        _pass(log, f"stream, decode group {db}", _loader(split, 64, False, True, db), pixels)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--content", default="noise,smooth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_stream.log"))
    ap.add_argument("--step", default=None, metavar="DIR")
    ap.add_argument("--legs", default="feed,test,train,sweep")
    ap.add_argument("--limit", type=int, default=420, help="seconds one content's child process may take")
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.out, a.legs)

    n = a.frames

    def log(s=""):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    tmp = tempfile.mkdtemp(prefix="stream_bench_")
    try:
        log()
        log(f"tools/bench_stream.py --frames {n} --content {a.content} on one MI355X ({time.strftime('%Y-%m-%d')}); seeded {H}x{W} 8-bit grey "
            "frames written as PNG by PIL, two label rows each; files written just before and read back once (reads come from the page cache, "
            "not from a disk)")
        log(f"every row = one pass over all frames with loaders of its own, in one process per content, in the order written: the DataLoader with "
            f"{CPUS} persistent spawn workers (PIL), the device image stream with {CPUS} reader threads (decode group {DEFAULT_BATCH} unless "
            "stated) twice, the workers again; seconds on the host clock from iter() to the final device synchronise, worker start-up and "
            "the stream's allocations included; first batch = until the first batch was on the device")
        for content in a.content.split(","):
            d = os.path.join(tmp, content)
            os.makedirs(os.path.join(d, "images"))
            os.makedirs(os.path.join(d, "labels"))
            with ProcessPoolExecutor(CPUS) as ex:
                list(ex.map(_write, [(os.path.join(d, "images"), lo, hi, content) for lo, hi in _spans(n, CPUS * 4)]))
            size = 0
            for f in os.listdir(os.path.join(d, "images")):
                with open(os.path.join(d, "images", f), "rb") as fh:
                    size += len(fh.read())
                with open(os.path.join(d, "labels", f[:-4] + ".txt"), "w") as fh:
                    fh.write("1 0.5 0.5 0.1 0.1\n2 0.25 0.75 0.2 0.1\n")   # (two rows: the csv sniffer takes the only line of a one-line file for a header)
            log(f"content {content}: {n} files, {size / n / 1e3:.0f} kB each = {100 * size / n / (H * W):.1f} % of the pixels")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", d, "--out", a.out, "--legs", a.legs], timeout=a.limit)
            except subprocess.TimeoutExpired:
                log(f"content {content}: no result within its limit of {a.limit} s")
                return 1
            if r.returncode != 0:
                log(f"content {content}: failed with exit status {r.returncode}")
                return 1
            shutil.rmtree(d, ignore_errors=True)
        return 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
