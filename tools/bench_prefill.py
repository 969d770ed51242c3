"""The prefill of the device image cache on one MI355X: the device decoder (`yogo train --device-image-cache GIB
--device-image-decode`: yogo_amd/png_prefill.py, csrc/inflate.hip, csrc/png_unpack_planes.hip) against the pool of PIL workers, in the
same run on the same machine.

Input: --frames seeded 772 x 1032 8-bit grey frames written as PNG by PIL (its default settings) with two label rows each, in the two
contents of tools/bench_png_feed.py (`noise`, `smooth`), into a temporary directory that is removed at the end.  The files are read
back once before anything is timed (they come from the page cache, not from a disk).  Every measurement is one
``ImageCache.prefill()`` of all frames in a child process of its own with its own time limit (``prefill_seconds``: the host clock
from the call to the final device synchronise, worker start-up included -- what a training run waits for); a step that fails or
runs out of time is recorded as such and no further step is started.  The lines are APPENDED to --out.

  host W      the one-off DataLoader with W spawn workers (16: a single rank's share of this machine's CPUs; 2: the share a rank
              has on an 8-rank node)
  device D    decode_batch D (the four sizes in turn, three times over): images/s, the device-event times of the yogo_inflate_zlib and yogo_png_unpack_planes launches per
              chunk, the scratch bytes (device: stored streams + scanlines; pinned: the two slots)

  python tools/bench_prefill.py [--frames 4096] [--content noise,smooth] [--out profiles/prefill_decode.log]

--leg resize: the same frames into a cache of 386 x 516 (`--image-hw 386 516`: an exact 2 x down-scale of every file), in the same run
the host prefill with 16 workers, the device prefill WITHOUT --device-image-resize (every file goes through ``image_uint8`` on the
prefill's threads) and WITH it (yogo_amd/png_prefill.py's groups, csrc/resize_aa.hip), the device rows three times each: images/s per
route, the device-event time of every yogo_resize_aa_u8 launch and its bytes in plus bytes out per second against the HBM peak.

  python tools/bench_prefill.py --leg resize [--frames 2048] --out profiles/prefill_resize.log
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

from bench_png_feed import CLASSES, H, W, _spans, _write   # noqa: E402  (the frame sets of the inference feed's benchmark)

WRITERS = 16
HOST_WORKERS = (16, 2)
DECODE_BATCHES = (256, 1024, 2048, 4096)
DEFAULT_BATCH = 1024   # yogo_amd.png_prefill.DEFAULT_DECODE_BATCH
REPEATS = 3
RESIZE_HW = (386, 516)
HBM_PEAK = 8.0e12   # bytes/s, MI355X


def step_prefill(d: str, route: str, arg: int, hw=(H, W)) -> dict:
    """route: host (arg workers), device (decode_batch arg) or device-resize (the same with device_resize=True); hw: the cache's size"""
    import torch

    from yogo_amd.image_cache import ImageCache
    from yogo_amd.resize import resize_aa_host
    from yogo_amd.yogo_dataset import ObjectDetectionDataset, read_image

    hw = (int(hw[0]), int(hw[1]))
    split = ObjectDetectionDataset(os.path.join(d, "images"), os.path.join(d, "labels"), 129, 97, CLASSES, image_hw=hw)
    n = len(split)
    torch.zeros(1, device="cuda")   # the device is up before the clock starts, as in a training run
    kw = dict(num_workers=arg) if route == "host" else dict(device_decode=True, decode_batch=arg, device_resize=route == "device-resize")
    cache = ImageCache(split, n, (1, *hw), False, device="cuda", batch_size=64, **kw)
    cache.prefill()

    def want(k):   # what the route is to hold: the host's bytes, or (device-resize) those of the kernel's numpy twin
        px = read_image(str(split._image_paths[k]))
        return torch.from_numpy(resize_aa_host(px.numpy(), hw)) if route == "device-resize" else split.image_uint8(k)

    ok = bool(cache.resident.all()) and int(cache.row_offsets[-1]) == sum(int(split.label_rows(k).shape[0]) for k in range(n)) == 2 * n and \
        all(torch.equal(cache.images[k].cpu(), want(k)) for k in (0, n // 2, n - 1))
    res = {"frames": n, "seconds": cache.prefill_seconds, "equals_read_image": ok, "checksum": int(cache.images.sum(dtype=torch.int64))}
    if route != "host":
        res.update(cache.decode_stats)
    return res


def leg_resize(log, d: str, n: int) -> bool:
    """the resize leg over one directory of frames -> False when a step gave no result"""
    hw = ["--hw", RESIZE_HW[0], RESIZE_HW[1]]
    r = run_step(log, 420, [d, "host", HOST_WORKERS[0]] + hw)
    if r is None:
        return False
    log(f"  host   {HOST_WORKERS[0]:>4d} workers, resize on the host         {r['seconds']:7.2f} s = {n / r['seconds']:7.0f} img/s   "
        f"(process {r['process_seconds']:.1f} s; equals image_uint8: {r['equals_read_image']}; checksum {r['checksum']})")
    for route, text in (("device", "resize on the host (threads)"), ("device-resize", "resize on the device       ")) * REPEATS:
        r = run_step(log, 420, [d, route, DEFAULT_BATCH] + hw)
        if r is None:
            return False
        log(f"  device {DEFAULT_BATCH:>4d} per chunk, {text} {r['seconds']:7.2f} s = {n / r['seconds']:7.0f} img/s   (process "
            f"{r['process_seconds']:.1f} s; equals {'the numpy twin' if route == 'device-resize' else 'image_uint8'}: {r['equals_read_image']}; "
            f"decoded on the host: {r['host_decoded']}, resized on the device: {r['device_resized']}; checksum {r['checksum']})")
        if route == "device-resize":
            inf, unp, rs = r["inflate_ms"], r["unpack_ms"], r["resize_ms"]
            per = min(DEFAULT_BATCH, n)
            moved = per * (H * W + RESIZE_HW[0] * RESIZE_HW[1])   # (the full chunks; the last one may be shorter, its time too)
            log(f"         {len(rs)} resize launches: {_med(rs):6.2f} ms median ({min(rs):.2f} .. {max(rs):.2f}) = {moved / _med(rs) / 1e9:6.2f} TB/s in "
                f"plus out = {100 * moved / (_med(rs) * 1e-3) / HBM_PEAK:.0f} % of the HBM peak; beside inflate {_med(inf):.1f} ms and unpack "
                f"{_med(unp):.1f} ms (its launches for the cache's own size and for the staging together: the latter is not timed); scratch "
                f"{r['scratch_device_bytes'] / 2 ** 30:.2f} GiB device + {r['scratch_pinned_bytes'] / 2 ** 30:.2f} GiB pinned")
    return True


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


def _med(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--content", default="noise,smooth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_decode.log"))
    ap.add_argument("--step", nargs=3, default=None, metavar=("DIR", "ROUTE", "ARG"))
    ap.add_argument("--hw", nargs=2, type=int, default=(H, W), help="(with --step) the cache's image size")
    ap.add_argument("--leg", choices=["decode", "resize"], default="decode")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_prefill(a.step[0], a.step[1], int(a.step[2]), a.hw)), flush=True)
        return 0

    n = a.frames

    def log(s=""):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    tmp = tempfile.mkdtemp(prefix="prefill_bench_")
    try:
        log()
        log(f"tools/bench_prefill.py --frames {n} --content {a.content} on one MI355X ({time.strftime('%Y-%m-%d')}); seeded {H}x{W} 8-bit grey "
            f"frames written as PNG by PIL, two label rows each; files written just before and read back once (reads come from the page cache, "
            "not from a disk)")
        log("every row = one ImageCache.prefill() of all frames in a process of its own: seconds on the host clock from the call to the final "
            "device synchronise (worker start-up included), images/s = frames / seconds; host W = the one-off DataLoader with W spawn "
            "workers; device D = yogo_amd/png_prefill.py with decode_batch D, the median and the range of the device-event times of the "
            "yogo_inflate_zlib and yogo_png_unpack_planes launches per chunk, and the scratch that lives during the prefill only")
        if a.leg == "resize":
            log(f"--leg resize: the cache at {RESIZE_HW[0]} x {RESIZE_HW[1]} (every file scaled down by 2); device rows: decode_batch {DEFAULT_BATCH}, "
                "without --device-image-resize (every file through image_uint8 on the prefill's threads: PIL, then resize_image) and with it "
                "(yogo_resize_aa_u8, one launch per chunk: its device-event times, and bytes in plus bytes out per second)")
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
                    fh.write("1 0.5 0.5 0.1 0.1\n2 0.25 0.75 0.2 0.1\n")   # (two rows: the loader's csv sniffer takes the only line of a one-line file for a header)
            if a.leg == "resize":
                log(f"content {content}: {n} files, {size / n / 1e3:.0f} kB each; --leg resize: the cache holds them at {RESIZE_HW[0]} x "
                    f"{RESIZE_HW[1]} = {n * RESIZE_HW[0] * RESIZE_HW[1] / 2 ** 30:.2f} GiB")
                if not leg_resize(log, d, n):
                    return 1
                shutil.rmtree(d, ignore_errors=True)
                continue
            log(f"content {content}: {n} files, {size / n / 1e3:.0f} kB each = {100 * size / n / (H * W):.1f} % of the pixels; the cache holds "
                f"{n * H * W / 2 ** 30:.2f} GiB")
            sums = set()
            for w in HOST_WORKERS:
                r = run_step(log, 900, [d, "host", w])
                if r is None:
                    return 1
                sums.add(r["checksum"])
                log(f"  host   {w:>4d} workers      {r['seconds']:7.2f} s = {n / r['seconds']:7.0f} img/s   (process {r['process_seconds']:.1f} s; "
                    f"equals read_image: {r['equals_read_image']})")
            for db in DECODE_BATCHES * REPEATS:   # (the sweep REPEATS times over, so that the rows of one chunk size show their spread)
                r = run_step(log, 600, [d, "device", db])
                if r is None:
                    return 1
                sums.add(r["checksum"])
                inf, unp = r["inflate_ms"], r["unpack_ms"]
                per = min(db, n)
                log(f"  device {db:>4d} per chunk    {r['seconds']:7.2f} s = {n / r['seconds']:7.0f} img/s   (process {r['process_seconds']:.1f} s; "
                    f"equals read_image: {r['equals_read_image']}; decoded on the host: {r['host_decoded']})")
                log(f"         {len(inf)} chunks: inflate {_med(inf):8.1f} ms median ({min(inf):.1f} .. {max(inf):.1f}) = {per / _med(inf) * 1e3:7.0f} img/s in the "
                    f"kernel, unpack {_med(unp):7.1f} ms median ({min(unp):.1f} .. {max(unp):.1f}) = {per / _med(unp) * 1e3:7.0f} img/s; scratch "
                    f"{r['scratch_device_bytes'] / 2 ** 30:.2f} GiB device + {r['scratch_pinned_bytes'] / 2 ** 30:.2f} GiB pinned")
            log(f"         all {len(HOST_WORKERS) + REPEATS * len(DECODE_BATCHES)} prefills sum the same pixels: {len(sums) == 1}")
            shutil.rmtree(d, ignore_errors=True)
        return 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
