"""Zarr input for inference on one MI355X: the feed alone, the unpack kernel alone, and `predict` against a PNG directory.

Input: 2048 seeded 772 x 1032 uint8 frames (a smooth background plus Gaussian noise of sigma 6, as tools/bench_loader.py), written
once to a scratch file and from there into each store (tests/_zarr_write.py's layout rules) and into a PNG directory; everything
lies in a temporary directory that is removed at the end.  Every measurement is a step in a child process of its own with its own
time limit; a step that fails or runs out of time is recorded as such, and no further step is started.

  (a) feed     ZarrDeviceFeed alone, batch 256, images/s on the host clock up to the final device synchronise (one warm-up
               pass, then the timed passes): (H, W, 1) raw zip, (H, W, 1) zlib zip, (H, W, 16) raw zip (deinterleave)
  (b) kernel   yogo_zarr_unpack alone from device events, B = 256, against the bytes it has to move (frame bytes read + output
               bytes written) as a share of 8 TB/s
  (c) predict  predict(count_predictions=True, half=True, batch_size=256) from the raw zip and from the same frames as a PNG
               directory (16 workers), alternated in one process, host clock around the whole call

  python tools/bench_zarr_feed.py [--frames 2048] [--out profiles/zarr_feed.log]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zipfile
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, B, WORKERS = 772, 1032, 256, 16
HBM_PEAK = 8.0e12
CLASSES = ["you", "only", "glance", "once"]


def _frame(k: int) -> np.ndarray:
    rng = np.random.default_rng(k)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    a, b, c = rng.uniform(0.5, 2.0, 3)
    smooth = 150 + 40 * np.sin(x / W * np.pi * a + c) * np.cos(y / H * np.pi * b)
    return np.clip(smooth + rng.normal(0, 6, size=(H, W)), 0, 255).astype(np.uint8)


def _frames(d: str, n: int) -> np.ndarray:
    return np.memmap(os.path.join(d, "frames.u8"), dtype=np.uint8, mode="r", shape=(n, H, W))


def _gen(args):
    d, n, lo, hi = args
    m = np.memmap(os.path.join(d, "frames.u8"), dtype=np.uint8, mode="r+", shape=(n, H, W))
    for k in range(lo, hi):
        m[k] = _frame(k)
    m.flush()


def _png(args):
    from PIL import Image

    d, n, lo, hi = args
    m = _frames(d, n)
    for k in range(lo, hi):
        Image.fromarray(np.asarray(m[k]), mode="L").save(os.path.join(d, "png", f"img_{k:04d}.png"))


def _chunk(args):
    d, n, t, cn, compress = args
    m = _frames(d, n)
    block = np.zeros((H, W, cn), dtype=np.uint8)
    for j in range(cn):
        if t * cn + j < n:
            block[:, :, j] = m[t * cn + j]
    raw = block.tobytes()
    return t, (zlib.compress(raw, 1) if compress else raw)


def _spans(n, parts):
    step = -(-n // parts)
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def write_store(d: str, n: int, name: str, cn: int, compress: bool) -> str:
    """an [H, W, n] array in (H, W, cn) chunks as a zip store of stored members"""
    p = os.path.join(d, name)
    meta = {"zarr_format": 2, "shape": [H, W, n], "chunks": [H, W, cn], "dtype": "|u1", "order": "C", "fill_value": 0, "filters": None,
            "compressor": {"id": "zlib", "level": 1} if compress else None, "dimension_separator": "."}
    with zipfile.ZipFile(p, "w", zipfile.ZIP_STORED) as zf, ProcessPoolExecutor(WORKERS) as ex:
        zf.writestr(".zarray", json.dumps(meta))
        for t, data in ex.map(_chunk, [(d, n, t, cn, compress) for t in range(-(-n // cn))], chunksize=2):
            zf.writestr(f"0.0.{t}", data)
    return p


# ---- the steps (child processes) ------------------------------------------------------------------------------------------

def step_feed(store: str, n: int, passes: int = 2) -> dict:
    import torch

    from yogo_amd.image_path_dataset import ZarrDataset
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    ds = ZarrDataset(store)
    rates, setup = [], []
    for p in range(passes + 1):
        t0 = time.perf_counter()
        feed = ZarrDeviceFeed(ds, B, "cuda", num_frames=n)   # allocates the pinned and the device buffers
        torch.cuda.synchronize()
        setup.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        seen, acc = 0, 0
        for x, names in feed:
            seen += x.shape[0]
            last = x
        acc = int(last[-1, 0, -1, -1])   # reads the last batch back: the device has finished
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert seen == n, (seen, n)
        if p:
            rates.append(n / dt)
    return {"images_per_s": rates, "setup_s": setup[1:], "bytes_on_disk": os.path.getsize(store), "last_pixel": acc}


def step_kernel() -> list:
    import torch

    from yogo_amd import _hip
    from yogo_amd.zarr_feed import ALIGN, unpack

    out = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for cn in (1, 16):
        stride = -(-(H * W * cn) // ALIGN) * ALIGN
        nchunks = B // cn
        staged = torch.randint(0, 256, (nchunks * stride,), dtype=torch.uint8, device="cuda", generator=g)
        toff = (np.arange(B, dtype=np.int64) // cn * stride).reshape(B, 1, 1)
        tk = (np.arange(B) % cn).astype(np.int32)
        toff_d, tk_d = torch.from_numpy(toff).cuda(), torch.from_numpy(tk).cuda()
        for dt in (torch.uint8, torch.float32):
            o = torch.empty((B, 1, H, W), dtype=dt, device="cuda")
            run = lambda: unpack(staged, toff, tk, chunks=(H, W, cn), order_f=False, fill=0, frame_shape=(H, W), out=o,  # noqa: E731
                                 tile_off_dev=toff_d, tile_k_dev=tk_d)
            _hip.launch_log(True)
            run()
            name = _hip.read_launch_log()[0].split(" | ")[0]
            _hip.launch_log(False)
            for _ in range(5):
                run()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
            ev[0].record()
            for i in range(20):
                run()
                ev[i + 1].record()
            torch.cuda.synchronize()
            us = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(20))
            moved = B * H * W * (1 + o.element_size())
            # what it computed, against the host's slicing
            k = B - 3
            chunk = staged[int(toff[k, 0, 0]):int(toff[k, 0, 0]) + H * W * cn].view(H, W, cn)[:, :, int(tk[k])]
            ok = bool(torch.equal(o[k, 0], chunk if dt == torch.uint8 else (chunk.cpu() / 255).cuda()))
            out.append({"kernel": name, "cn": cn, "median_us": us[10], "min_us": us[0], "bytes_moved": moved,
                        "share_of_8TBps": moved / (us[10] * 1e-6) / HBM_PEAK, "matches_host": ok})
    return out


def step_predict(d: str, store: str, n: int) -> dict:
    import contextlib
    import io

    import torch

    from yogo_amd.infer import predict
    from yogo_amd.model import YOGO

    torch.manual_seed(3)
    net = YOGO((H, W), 0.0425, 0.0555, 4).cuda().eval()
    pth = os.path.join(d, "m.pth")
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "bench",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, pth)
    del net
    res = {"zarr_s": [], "png_s": [], "counts": []}
    for rep in range(2):
        for kind in ("zarr", "png"):
            buf = io.StringIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(buf):
                if kind == "zarr":
                    predict(pth, path_to_zarr=store, count_predictions=True, half=True, batch_size=B, class_names=CLASSES)
                else:
                    predict(pth, path_to_images=os.path.join(d, "png"), count_predictions=True, half=True, batch_size=B,
                            class_names=CLASSES, requested_num_workers=WORKERS)
            torch.cuda.synchronize()
            res[kind + "_s"].append(time.perf_counter() - t0)
            res["counts"].append(buf.getvalue().strip().splitlines()[-1])
    res["same_counts"] = len(set(res["counts"])) == 1
    res["counts"] = res["counts"][0]
    res["frames"] = n
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
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zarr_feed.log"))
    ap.add_argument("--step", default=None)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    if a.step:
        if a.step == "feed":
            res = step_feed(a.rest[0], int(a.rest[1]))
        elif a.step == "kernel":
            res = step_kernel()
        else:
            res = step_predict(a.rest[0], a.rest[1], int(a.rest[2]))
        print("RESULT " + json.dumps(res), flush=True)
        return 0

    n = a.frames
    lines = []

    def log(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    d = tempfile.mkdtemp(prefix="zarr_bench_")
    try:
        log(f"tools/bench_zarr_feed.py --frames {n} on one MI355X; {n} seeded {H}x{W} uint8 frames (smooth background + Gaussian noise "
            f"sigma 6), batch {B}")
        np.memmap(os.path.join(d, "frames.u8"), dtype=np.uint8, mode="w+", shape=(n, H, W)).flush()
        with ProcessPoolExecutor(WORKERS) as ex:
            list(ex.map(_gen, [(d, n, lo, hi) for lo, hi in _spans(n, WORKERS * 4)]))
        log()
        log("(a) ZarrDeviceFeed alone: read -> pinned staging -> upload -> unpack, images/s on the host clock, timed passes after a warm-up pass;")
        log("    the stores were written just before: reads come from the page cache, not from a disk")
        ok = True
        raw_store = None
        for label, name, cn, compress in (("(H, W, 1) raw zip ", "raw1.zip", 1, False), ("(H, W, 1) zlib zip", "zlib1.zip", 1, True),
                                          ("(H, W, 16) raw zip", "raw16.zip", 16, False)):
            store = write_store(d, n, name, cn, compress)
            r = run_step(log, "feed", 240, [store, n])
            if r is None:
                ok = False
                break
            log(f"  {label}  " + "  ".join(f"{v:9.0f} img/s" for v in r["images_per_s"]) + f"   ({r['bytes_on_disk'] / n / (H * W) * 100:.1f} % "
                f"of raw on disk; buffers allocated in {max(r['setup_s']):.2f} s before each pass, not counted)")
            if name == "raw1.zip":
                raw_store = store
            else:
                os.remove(store)
        if ok:
            log()
            log(f"(b) yogo_zarr_unpack alone, B = {B}, device events around each of 20 launches (median / min), bytes = frames read + output written")
            r = run_step(log, "kernel", 180, [])
            ok = r is not None
            for k in r or []:
                log(f"  {k['kernel']:<42s} cn={k['cn']:<3d} {k['median_us']:8.1f} us / {k['min_us']:8.1f} us   {k['bytes_moved'] / 1e6:7.1f} MB   "
                    f"{k['bytes_moved'] / (k['median_us'] * 1e-6) / 1e12:5.2f} TB/s = {k['share_of_8TBps'] * 100:4.1f} % of 8 TB/s"
                    f"   equals the host's slicing: {k['matches_host']}")
        if ok:
            os.makedirs(os.path.join(d, "png"))
            with ProcessPoolExecutor(WORKERS) as ex:
                list(ex.map(_png, [(d, n, lo, hi) for lo, hi in _spans(n, WORKERS * 4)]))
            log()
            log(f"(c) predict(count_predictions=True, half=True, batch_size={B}) over the {n} frames, host clock around the whole call (model load "
                "included), zarr and PNG alternated twice in one process; PNG directory read by 16 DataLoader workers")
            r = run_step(log, "predict", 420, [d, raw_store, n])
            if r is not None:
                for kind, label in (("zarr", "(H, W, 1) raw zip"), ("png", "PNG directory    ")):
                    log(f"  {label}  " + "  ".join(f"{s:7.2f} s = {n / s:8.0f} img/s" for s in r[kind + "_s"]))
                log(f"  the four runs print the same counts: {r['same_counts']}   {r['counts']}")
        return 0
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
