"""PNG directories for inference on one MI355X: the device image decoder (`yogo infer --device-image-decode`:
yogo_amd/png_feed.py, csrc/inflate.hip, csrc/png_unpack.hip) against the DataLoader route, in the same run on the same machine.

Input: --frames seeded 772 x 1032 8-bit grey frames written as PNG by PIL (its default settings) into a temporary directory that
is removed at the end, in two contents: `noise` = sensor-noise-like (Gaussian noise of sigma 25 round a flat level: PNG hardly
shrinks it), `smooth` = a smooth background plus Gaussian noise of sigma 6 (as tools/bench_zarr_feed.py).  The files are read back
once before anything is timed (they come from the page cache, not from a disk).  Every measurement is a step in a child process
of its own with its own time limit; a step that fails or runs out of time is recorded as such and no further step is started.
The lines are APPENDED to --out.

  feed     batch 256, images/s on the host clock up to the final device synchronise; `device` = PngDeviceFeed, `host` = the
           DataLoader predict() builds (16 workers, pinned, collate) plus the upload of every batch; one warm-up pass of each,
           then --passes timed passes of each, alternated
  kernels  yogo_inflate_zlib and yogo_png_unpack alone on the first batch, device events around each of 5 launches
  predict  predict(count_predictions=True, half=True, device_outputs=True, batch_size=256), host clock around the whole call
           (model load included), device_image_decode on and off, alternated, twice each

  python tools/bench_png_feed.py [--frames 1024] [--content noise,smooth] [--out profiles/png_feed.log]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, B, WORKERS = 772, 1032, 256, 16
CLASSES = ["you", "only", "glance", "once"]


def _frame(k: int, content: str) -> np.ndarray:
    rng = np.random.default_rng(k)
    if content == "noise":
        return np.clip(rng.normal(110, 25, size=(H, W)), 0, 255).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    a, b, c = rng.uniform(0.5, 2.0, 3)
    smooth = 150 + 40 * np.sin(x / W * np.pi * a + c) * np.cos(y / H * np.pi * b)
    return np.clip(smooth + rng.normal(0, 6, size=(H, W)), 0, 255).astype(np.uint8)


def _write(args):
    from PIL import Image

    d, lo, hi, content = args
    for k in range(lo, hi):
        Image.fromarray(_frame(k, content), mode="L").save(os.path.join(d, f"img_{k:05d}.png"))


def _spans(n, parts):
    step = -(-n // parts)
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


# ---- the steps (child processes) ------------------------------------------------------------------------------------------

def step_feed(d: str, passes: int) -> dict:
    import torch
    from torch.utils.data import DataLoader

    from yogo_amd.image_path_dataset import ImagePathDataset, collate_fn
    from yogo_amd.png_feed import PngDeviceFeed

    ds = ImagePathDataset(d)
    n = len(ds)

    def run(route):
        t0 = time.perf_counter()
        if route == "device":
            it = PngDeviceFeed(ds, B, "cuda")
        else:
            it = DataLoader(ds, batch_size=B, shuffle=False, drop_last=False, pin_memory=True, collate_fn=collate_fn, num_workers=WORKERS)
        seen, total = 0, 0
        for x, names in it:
            x = x.to("cuda", non_blocking=True)
            seen += x.shape[0]
            total += int(x[-1, 0, -1, -1])   # reads every batch's last pixel back: the device has finished with it
        torch.cuda.synchronize()
        assert seen == n, (seen, n)
        host = getattr(it, "host_decoded", None)
        return n / (time.perf_counter() - t0), total, host

    res = {"device": [], "host": [], "frames": n}
    sums = set()
    for p in range(passes + 1):
        for route in ("device", "host"):
            rate, total, host = run(route)
            sums.add(total)
            if p:
                res[route].append(rate)
            if route == "device":
                res["host_decoded"] = host
    res["same_pixels"] = len(sums) == 1
    return res


def step_kernels(d: str) -> dict:
    """the two kernels alone on the first batch"""
    import torch

    from yogo_amd import inflate, png
    from yogo_amd.device_decode import inflate_streams, png_unpack
    from yogo_amd.image_path_dataset import ImagePathDataset
    from yogo_amd.yogo_dataset import read_image

    paths = [str(p) for p in ImagePathDataset(d).image_paths[:B]]
    stored, rows, table = bytearray(), [], []
    stride = -(-(H * (1 + W)) // 16) * 16
    for i, p in enumerate(paths):
        data = open(p, "rb").read()
        info = png.parse_png(data)
        assert info.device_decodable and (info.height, info.width) == (H, W)
        stream = b"".join(data[o:o + n] for o, n in info.idat)
        off, ln, adler = inflate.split_zlib(stream)
        rows.append((len(stored) + off, ln, i * stride, H * (1 + W), adler))
        table.append((i * stride, 0))
        stored += stream
    n = len(paths)
    src = torch.frombuffer(stored, dtype=torch.uint8).cuda()
    rows_d = torch.tensor(rows, dtype=torch.int64, device="cuda")
    table_d = torch.tensor(table, dtype=torch.int64, device="cuda")
    scan = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
    st_i = torch.empty(n, dtype=torch.int32, device="cuda")
    st_u = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.empty((n, 1, H, W), dtype=torch.uint8, device="cuda")
    times = {"inflate": [], "unpack": []}
    for rep in range(6):   # (the unpack writes into the scanlines: every launch of it follows an inflate)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        inflate_streams(src, rows_d, scan, st_i)
        ev[1].record()
        png_unpack(scan, table_d, (H, W), out, st_u)
        ev[2].record()
        torch.cuda.synchronize()
        if rep:
            times["inflate"].append(ev[0].elapsed_time(ev[1]) * 1e3)
            times["unpack"].append(ev[1].elapsed_time(ev[2]) * 1e3)
    ok = not bool(st_i.any()) and not bool(st_u.any()) and all(torch.equal(out[k].cpu(), read_image(paths[k])) for k in (0, n // 2, n - 1))
    return {"frames": n, "stored_bytes": len(stored), "inflated_bytes": n * H * (1 + W), "equals_read_image": ok,
            "inflate_us": sorted(times["inflate"]), "unpack_us": sorted(times["unpack"])}


def step_predict(d: str, tmp: str) -> dict:
    import contextlib
    import io

    import torch

    from yogo_amd.infer import predict
    from yogo_amd.model import YOGO

    torch.manual_seed(3)
    net = YOGO((H, W), 0.0425, 0.0555, 4).cuda().eval()
    pth = os.path.join(tmp, "m.pth")
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "bench",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, pth)
    del net
    res = {"device_s": [], "host_s": [], "counts": []}
    for rep in range(2):
        for route in ("device", "host"):
            buf = io.StringIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(buf):
                predict(pth, path_to_images=d, count_predictions=True, half=True, batch_size=B, class_names=CLASSES, device_outputs=True,
                        requested_num_workers=WORKERS, device_image_decode=route == "device")
            torch.cuda.synchronize()
            res[route + "_s"].append(time.perf_counter() - t0)
            res["counts"].append(buf.getvalue().strip().splitlines()[-1])
    res["same_counts"] = len(set(res["counts"])) == 1
    res["counts"] = res["counts"][0]
    return res


def run_step(log, name: str, limit: int, args: list):
    """one measurement in a child process of its own, under its own time limit -> its JSON result, or None"""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [str(a) for a in args]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        log(f"step {name} {args}: no result within its limit of {limit} s")
        return None
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        log(f"step {name} {args}: failed with exit status {r.returncode}\n{r.stderr[-2000:]}")
        return None
    log(f"  (step {name}: {time.perf_counter() - t0:.1f} s in its own process, limit {limit} s)")
    return json.loads(lines[-1][len("RESULT "):])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--content", default="noise,smooth")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_feed.log"))
    ap.add_argument("--step", default=None)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    if a.step:
        res = step_feed(a.rest[0], int(a.rest[1])) if a.step == "feed" else step_kernels(a.rest[0]) if a.step == "kernels" \
            else step_predict(a.rest[0], a.rest[1])
        print("RESULT " + json.dumps(res), flush=True)
        return 0

    n = a.frames

    def log(s=""):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    tmp = tempfile.mkdtemp(prefix="png_bench_")
    try:
        log()
        log(f"tools/bench_png_feed.py --frames {n} --content {a.content} --passes {a.passes} on one MI355X ({time.strftime('%Y-%m-%d')}); seeded "
            f"{H}x{W} 8-bit grey frames written as PNG by PIL, batch {B}, {WORKERS} CPUs; files written just before and read back once "
            "(reads come from the page cache, not from a disk)")
        log("feed = the batches alone, images/s on the host clock up to the final device synchronise, timed passes after a warm-up pass of "
            "each route, alternated; device = PngDeviceFeed (yogo_inflate_zlib + yogo_png_unpack), host = DataLoader with 16 workers + upload; "
            "kernels = the two kernels alone on the first batch, device events, sorted us of 5 launches; predict = predict(count_predictions, "
            "half, device_outputs), host clock around the whole call (model load included), alternated")
        for content in a.content.split(","):
            d = os.path.join(tmp, content)
            os.makedirs(d)
            with ProcessPoolExecutor(WORKERS) as ex:
                list(ex.map(_write, [(d, lo, hi, content) for lo, hi in _spans(n, WORKERS * 4)]))
            size = 0
            for f in os.listdir(d):
                with open(os.path.join(d, f), "rb") as fh:
                    size += len(fh.read())
            log(f"content {content}: {n} files, {size / n / 1e3:.0f} kB each = {100 * size / n / (H * W):.1f} % of the pixels")
            r = run_step(log, "feed", 600, [d, a.passes])
            if r is None:
                return 1
            for route in ("device", "host"):
                log(f"  feed     {route:<6s} " + "  ".join(f"{v:9.0f} img/s" for v in r[route]))
            log(f"           the passes of both routes sum the same pixels: {r['same_pixels']}; decoded on the host in the device route: {r['host_decoded']}")
            k = run_step(log, "kernels", 300, [d])
            if k is None:
                return 1
            med_i, med_u = k["inflate_us"][len(k["inflate_us"]) // 2], k["unpack_us"][len(k["unpack_us"]) // 2]
            log(f"  kernels  yogo_inflate_zlib " + " ".join(f"{v:9.0f}" for v in k["inflate_us"]) + f" us per batch of {k['frames']}: "
                f"{k['stored_bytes'] / 1e6:.1f} MB stored -> {k['inflated_bytes'] / 1e6:.1f} MB = {k['inflated_bytes'] / (med_i * 1e-6) / 1e9:.1f} GB/s out, "
                f"{k['frames'] / (med_i * 1e-6):.0f} img/s")
            log(f"           yogo_png_unpack   " + " ".join(f"{v:9.0f}" for v in k["unpack_us"]) + f" us = {k['frames'] / (med_u * 1e-6):.0f} img/s; "
                f"images equal read_image: {k['equals_read_image']}")
            if not a.no_predict:
                r = run_step(log, "predict", 900, [d, tmp])
                if r is None:
                    return 1
                for route in ("device", "host"):
                    log(f"  predict  {route:<6s} " + "  ".join(f"{t:7.2f} s = {n / t:8.0f} img/s" for t in r[route + "_s"]))
                log(f"           the four runs print the same counts: {r['same_counts']}   {r['counts']}")
            shutil.rmtree(d, ignore_errors=True)
        return 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
