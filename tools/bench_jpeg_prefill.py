"""The prefill of the device image cache from JPEG files on one MI355X (`--device-image-decode-jpeg`: yogo_amd/png_prefill.py,
csrc/jpeg_decode.hip) against the pool of PIL workers and against the device prefill without the switch, in the same run on the
same machine.  tools/bench_prefill.py's frame sets and its way of measuring -- every row one ``ImageCache.prefill()`` of all frames in
a child process of its own under its own time limit; a step that fails or runs out of time is recorded and no further step is
started --, the files written as JPEG: 772 x 1032, 8-bit grey, quality 90, by PIL, two label rows each.

  host W        the one-off DataLoader with W spawn workers (16, 2)
  device        decode_batch 1024 without the switch: every JPEG through PIL on the prefill's threads (three runs)
  device-jpeg D decode_batch D (1024 three times, 256 once) with the switch: images/s, the device-event times of the
                yogo_jpeg_decode launch per chunk, files handed back to the host

  python tools/bench_jpeg_prefill.py [--frames 2048] [--content noise,smooth] [--out profiles/jpeg_feed.log]
"""
import argparse
import json
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

from bench_png_feed import CLASSES, H, W, _frame, _spans   # noqa: E402
from bench_prefill import HOST_WORKERS, REPEATS, WRITERS, _med   # noqa: E402

QUALITY = 90


def _write(args):
    from PIL import Image

    d, lo, hi, content = args
    for k in range(lo, hi):
        Image.fromarray(_frame(k, content), mode="L").save(os.path.join(d, f"img_{k:05d}.jpg"), format="JPEG", quality=QUALITY)


def step_prefill(d: str, route: str, arg: int) -> dict:
    """route: host (arg workers), device (decode_batch arg, every JPEG on the prefill's threads) or device-jpeg (the switch on)"""
    import torch

    from yogo_amd.image_cache import ImageCache
    from yogo_amd.yogo_dataset import ObjectDetectionDataset

    split = ObjectDetectionDataset(os.path.join(d, "images"), os.path.join(d, "labels"), 129, 97, CLASSES, image_hw=(H, W))
    n = len(split)
    torch.zeros(1, device="cuda")
    kw = dict(num_workers=arg) if route == "host" else dict(device_decode=True, decode_batch=arg, device_decode_jpeg=route == "device-jpeg")
    cache = ImageCache(split, n, (1, H, W), False, device="cuda", batch_size=64, **kw)
    cache.prefill()
    ok = bool(cache.resident.all()) and int(cache.row_offsets[-1]) == 2 * n and \
        all(torch.equal(cache.images[k].cpu(), split.image_uint8(k)) for k in (0, n // 2, n - 1))
    res = {"frames": n, "seconds": cache.prefill_seconds, "equals_read_image": ok, "checksum": int(cache.images.sum(dtype=torch.int64))}
    if route != "host":
        res.update(cache.decode_stats)
    return res


def run_step(log, limit: int, args: list):
    """one measurement in a child process of its own, under its own time limit -> its JSON result, or None"""
    cmd = [sys.executable, os.path.abspath(__file__), "--step"] + [str(a) for a in args]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        log(f"step {args[1:]}: no result within its limit of {limit} s")
        return None
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        log(f"step {args[1:]}: failed with exit status {r.returncode}\n{r.stderr[-2000:]}")
        return None
    res = json.loads(lines[-1][len("RESULT "):])
    res["process_seconds"] = time.perf_counter() - t0
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--content", default="noise,smooth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_feed.log"))
    ap.add_argument("--step", nargs=3, default=None, metavar=("DIR", "ROUTE", "ARG"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_prefill(a.step[0], a.step[1], int(a.step[2]))), flush=True)
        return 0
    n = a.frames

    def log(s=""):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    tmp = tempfile.mkdtemp(prefix="jpeg_prefill_bench_")
    try:
        log()
        log(f"tools/bench_jpeg_prefill.py --frames {n} --content {a.content} on one MI355X ({time.strftime('%Y-%m-%d')}); seeded {H}x{W} 8-bit "
            f"grey frames written as JPEG (quality {QUALITY}, baseline, no restart markers) by PIL, two label rows each; files written just "
            "before and read back once (reads come from the page cache, not from a disk)")
        log("every row = one ImageCache.prefill() of all frames in a process of its own: seconds on the host clock from the call to the "
            "final device synchronise (worker start-up included); host W = the one-off DataLoader with W spawn workers; device = "
            "--device-image-decode without --device-image-decode-jpeg (every file through PIL on the prefill's threads); device-jpeg D = "
            "with it, decode_batch D: the device-event times of the yogo_jpeg_decode launch per chunk")
        for content in a.content.split(","):
            d = os.path.join(tmp, content)
            os.makedirs(os.path.join(d, "images"))
            os.makedirs(os.path.join(d, "labels"))
            with ProcessPoolExecutor(WRITERS) as ex:
                list(ex.map(_write, [(os.path.join(d, "images"), lo, hi, content) for lo, hi in _spans(n, WRITERS * 4)]))
            size = 0
            for f in os.listdir(os.path.join(d, "images")):
                with open(os.path.join(d, "images", f), "rb") as fh:
                    size += len(fh.read())
                with open(os.path.join(d, "labels", f[:-4] + ".txt"), "w") as fh:
                    fh.write("1 0.5 0.5 0.1 0.1\n2 0.25 0.75 0.2 0.1\n")
            log(f"content {content}: {n} files, {size / n / 1e3:.0f} kB each = {100 * size / n / (H * W):.1f} % of the pixels")
            sums = set()
            for w in HOST_WORKERS:
                r = run_step(log, 900, [d, "host", w])
                if r is None:
                    return 1
                sums.add(r["checksum"])
                log(f"  host        {w:>4d} workers    {r['seconds']:7.2f} s = {n / r['seconds']:7.0f} img/s   (process {r['process_seconds']:.1f} s; "
                    f"equals read_image: {r['equals_read_image']})")
            for route, db in (("device", 1024), ("device-jpeg", 1024)) * REPEATS + (("device-jpeg", 256),):
                r = run_step(log, 600, [d, route, db])
                if r is None:
                    return 1
                sums.add(r["checksum"])
                log(f"  {route:<11s} {db:>4d} per chunk  {r['seconds']:7.2f} s = {n / r['seconds']:7.0f} img/s   (process {r['process_seconds']:.1f} s; "
                    f"equals read_image: {r['equals_read_image']}; decoded on the host: {r['host_decoded']}"
                    + (f", by yogo_jpeg_decode: {r['jpeg_decoded']})" if route == "device-jpeg" else ")"))
                if route == "device-jpeg":
                    ms, unp = r["jpeg_ms"], r["unpack_ms"]
                    per = min(db, n)
                    log(f"         {len(ms)} chunks: yogo_jpeg_decode {_med(ms):8.1f} ms median ({min(ms):.1f} .. {max(ms):.1f}) = "
                        f"{per / _med(ms) * 1e3:7.0f} img/s in the kernel, unpack {_med(unp):6.1f} ms median; scratch "
                        f"{r['scratch_device_bytes'] / 2 ** 30:.2f} GiB device + {r['scratch_pinned_bytes'] / 2 ** 30:.2f} GiB pinned")
            log(f"         all {len(HOST_WORKERS) + 2 * REPEATS + 1} prefills sum the same pixels: {len(sums) == 1}")
            shutil.rmtree(d, ignore_errors=True)
        return 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
