"""PNG directories of other formats than 8-bit grey for inference on one MI355X: `yogo infer --device-image-decode
--device-image-decode-all` (yogo_amd/png_feed.py with all_types, csrc/inflate.hip, csrc/png_unpack_any.hip) against what such a
directory gets without the new switch, in the same run on the same machine.  A sibling of tools/bench_png_feed.py (whose grey leg
stays the measurement of `yogo_png_unpack`).

Input: --frames seeded 772 x 1032 frames (the smooth background plus Gaussian noise of sigma 6 of tools/bench_png_feed.py) in a
temporary directory per format, removed at the end: `rgb8` (three such planes, PIL's writer), `palette8` (the frame as indices into
a 256-entry colour table, PIL's writer), `grey16` (the frame times 200 plus 8 bits of noise, PIL's writer), `grey8_adam7` (PIL
writes no interlaced files: the seven reduced images under filter type 0, zlib level 6).  The files are read back once before
anything is timed.  Every measurement is a step in a child process of its own with its own time limit; a step that fails or runs
out of time is recorded as such and no further step is started.  The lines are APPENDED to --out.

  feed     batch 256 into a one-plane model's batches, images/s on the host clock up to the final device synchronise:
           `all`    = PngDeviceFeed(all_types=True), three timed passes after a warm-up pass;
           `decode` = PngDeviceFeed alone (--device-image-decode without the new switch: every file falls back to PIL on the
                      feed's 16 threads), one timed pass;
           `loader` = the DataLoader predict() builds (16 workers, pinned, collate) plus the upload, one timed pass after a warm-up
  kernels  yogo_inflate_zlib and yogo_png_unpack_any alone on the first batch, device events around each of 5 launches

  python tools/bench_png_types.py [--frames 1024] [--formats rgb8,palette8,grey16,grey8_adam7] [--out profiles/png_types.log]
"""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, B, WORKERS = 772, 1032, 256, 16
FORMATS = ("rgb8", "palette8", "grey16", "grey8_adam7")
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def _plane(rng) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    a, b, c = rng.uniform(0.5, 2.0, 3)
    smooth = 150 + 40 * np.sin(x / W * np.pi * a + c) * np.cos(y / H * np.pi * b)
    return np.clip(smooth + rng.normal(0, 6, size=(H, W)), 0, 255).astype(np.uint8)


def _chunk(ctype: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data))


def _write(args):
    from PIL import Image

    d, lo, hi, fmt = args
    for k in range(lo, hi):
        rng = np.random.default_rng(k)
        path = os.path.join(d, f"img_{k:05d}.png")
        if fmt == "rgb8":
            Image.fromarray(np.stack([_plane(rng) for _ in range(3)], axis=2)).save(path)
        elif fmt == "palette8":
            im = Image.fromarray(_plane(rng))   # (putpalette makes it a palette image)
            im.putpalette(rng.integers(0, 256, size=768, dtype=np.uint8).tobytes())
            im.save(path)
        elif fmt == "grey16":
            Image.fromarray(_plane(rng).astype(np.uint16) * 200 + rng.integers(0, 256, size=(H, W), dtype=np.uint16)).save(path)
        else:
            px = _plane(rng)
            scan = bytearray()
            for x0, y0, dx, dy in ADAM7:
                sub = px[y0::dy, x0::dx]
                scan += np.concatenate((np.zeros((sub.shape[0], 1), np.uint8), sub), axis=1).tobytes()
            with open(path, "wb") as f:
                f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0, 0, 0, 1))
                        + _chunk(b"IDAT", zlib.compress(bytes(scan), 6)) + _chunk(b"IEND", b""))


def _spans(n, parts):
    step = -(-n // parts)
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


# ---- the steps (child processes) ------------------------------------------------------------------------------------------

def step_feed(d: str) -> dict:
    import torch
    from torch.utils.data import DataLoader

    from yogo_amd.image_path_dataset import ImagePathDataset, collate_fn
    from yogo_amd.png_feed import PngDeviceFeed

    ds = ImagePathDataset(d)
    n = len(ds)

    def run(route):
        t0 = time.perf_counter()
        if route == "all":
            it = PngDeviceFeed(ds, B, "cuda", all_types=True)
        elif route == "decode":
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
        return n / (time.perf_counter() - t0), total, getattr(it, "host_decoded", None)

    res = {"all": [], "decode": [], "loader": [], "frames": n}
    sums = set()
    for route, warm, timed in (("all", 1, 3), ("loader", 1, 1), ("decode", 0, 1)):
        for p in range(warm + timed):
            rate, total, host = run(route)
            sums.add(total)
            if p >= warm:
                res[route].append(rate)
            res[route + "_host_decoded"] = host
    res["same_pixels"] = len(sums) == 1
    return res


def step_kernels(d: str) -> dict:
    """the two kernels alone on the first batch"""
    import torch

    from yogo_amd import inflate, png
    from yogo_amd.device_decode import inflate_streams, png_unpack_any
    from yogo_amd.image_path_dataset import ImagePathDataset
    from yogo_amd.yogo_dataset import read_image

    paths = [str(p) for p in ImagePathDataset(d).image_paths[:B]]
    stored, rows, table, palettes, at = bytearray(), [], [], [], 0
    for i, p in enumerate(paths):
        data = open(p, "rb").read()
        info = png.parse_png(data)
        assert info.any_decodable and (info.height, info.width) == (H, W)
        stream = b"".join(data[o:o + n] for o, n in info.idat)
        off, ln, adler = inflate.split_zlib(stream)
        rows.append((len(stored) + off, ln, at, info.inflated_bytes, adler))
        table.append([at, info.format_code, 0])
        if info.color_type == 3:
            palettes.append((i, png.palette_table(data, info)))
        at += -(-info.inflated_bytes // 16) * 16
        stored += stream
    n, inflated = len(paths), sum(r[3] for r in rows)
    for k, (i, _) in enumerate(palettes):
        table[i][2] = at + k * png.PALETTE_BYTES
    src = torch.frombuffer(stored, dtype=torch.uint8).cuda()
    rows_d = torch.tensor(rows, dtype=torch.int64, device="cuda")
    table_d = torch.tensor(table, dtype=torch.int64, device="cuda")
    scan = torch.empty(at + len(palettes) * png.PALETTE_BYTES + 16, dtype=torch.uint8, device="cuda")
    if palettes:
        scan[at:at + len(palettes) * png.PALETTE_BYTES].copy_(torch.from_numpy(np.concatenate([t for _, t in palettes])))
    st_i = torch.empty(n, dtype=torch.int32, device="cuda")
    st_u = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.empty((n, 1, H, W), dtype=torch.uint8, device="cuda")
    times = {"inflate": [], "unpack": []}
    for rep in range(6):   # (the unpack writes into the scanlines: every launch of it follows an inflate)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        inflate_streams(src, rows_d, scan, st_i)
        ev[1].record()
        png_unpack_any(scan, table_d, (H, W), out, st_u)
        ev[2].record()
        torch.cuda.synchronize()
        if rep:
            times["inflate"].append(ev[0].elapsed_time(ev[1]) * 1e3)
            times["unpack"].append(ev[1].elapsed_time(ev[2]) * 1e3)
    ok = not bool(st_i.any()) and not bool(st_u.any()) and all(torch.equal(out[k].cpu(), read_image(paths[k])) for k in (0, n // 2, n - 1))
    return {"frames": n, "stored_bytes": len(stored), "inflated_bytes": inflated, "equals_read_image": ok,
            "inflate_us": sorted(times["inflate"]), "unpack_us": sorted(times["unpack"])}


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
    ap.add_argument("--formats", default=",".join(FORMATS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_types.log"))
    ap.add_argument("--step", default=None)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    if a.step:
        res = step_feed(a.rest[0]) if a.step == "feed" else step_kernels(a.rest[0])
        print("RESULT " + json.dumps(res), flush=True)
        return 0

    n = a.frames

    def log(s=""):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    tmp = tempfile.mkdtemp(prefix="png_types_bench_")
    try:
        log()
        log(f"tools/bench_png_types.py --frames {n} --formats {a.formats} on one MI355X ({time.strftime('%Y-%m-%d')}); seeded {H}x{W} frames, one "
            f"directory per format, batch {B}, {WORKERS} CPUs; files written just before and read back once (reads come from the page cache, "
            "not from a disk)")
        log("feed = one-plane batches alone, images/s on the host clock up to the final device synchronise; all = PngDeviceFeed(all_types=True) "
            "(yogo_inflate_zlib + yogo_png_unpack_any), three timed passes after a warm-up; decode = PngDeviceFeed without the switch (every "
            "file through PIL on the feed's 16 threads), one pass; loader = DataLoader with 16 workers + upload, one pass after a warm-up; "
            "kernels = the two kernels alone on the first batch, device events, sorted us of 5 launches")
        for fmt in a.formats.split(","):
            d = os.path.join(tmp, fmt)
            os.makedirs(d)
            with ProcessPoolExecutor(WORKERS) as ex:
                list(ex.map(_write, [(d, lo, hi, fmt) for lo, hi in _spans(n, WORKERS * 4)]))
            size = 0
            for f in os.listdir(d):
                with open(os.path.join(d, f), "rb") as fh:
                    size += len(fh.read())
            log(f"format {fmt}: {n} files, {size / n / 1e3:.0f} kB each")
            r = run_step(log, "feed", 900, [d])
            if r is None:
                return 1
            for route in ("all", "decode", "loader"):
                log(f"  feed     {route:<6s} " + "  ".join(f"{v:9.0f} img/s" for v in r[route])
                    + (f"   (decoded on the host: {r[route + '_host_decoded']})" if route != "loader" else ""))
            log(f"           the passes of all routes sum the same pixels: {r['same_pixels']}")
            k = run_step(log, "kernels", 300, [d])
            if k is None:
                return 1
            med_i, med_u = k["inflate_us"][len(k["inflate_us"]) // 2], k["unpack_us"][len(k["unpack_us"]) // 2]
            log(f"  kernels  yogo_inflate_zlib   " + " ".join(f"{v:9.0f}" for v in k["inflate_us"]) + f" us per batch of {k['frames']}: "
                f"{k['stored_bytes'] / 1e6:.1f} MB stored -> {k['inflated_bytes'] / 1e6:.1f} MB = {k['inflated_bytes'] / (med_i * 1e-6) / 1e9:.1f} GB/s out, "
                f"{k['frames'] / (med_i * 1e-6):.0f} img/s")
            log(f"           yogo_png_unpack_any " + " ".join(f"{v:9.0f}" for v in k["unpack_us"]) + f" us = {k['frames'] / (med_u * 1e-6):.0f} img/s; "
                f"images equal read_image: {k['equals_read_image']}")
            shutil.rmtree(d, ignore_errors=True)
        return 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
