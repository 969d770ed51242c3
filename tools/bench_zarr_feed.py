"""Zarr input for inference on one MI355X: the feed alone per compressor and decode route, the decode and unpack kernels alone,
and `predict` from each store (optionally against a PNG directory).

Input: seeded 772 x 1032 uint8 frames, written once to a scratch file and from there into each store (tests/_zarr_write.py's
layout rules) and, with --png, into a PNG directory; everything lies in a temporary directory that is removed at the end.
The zstd legs (`blosc-zstd`: Blosc with one Zstandard frame per block; `zstd`: the zstd codec, one frame per chunk) are written by the
system's libzstd through ctypes where it loads, else by tests/_zstd_write.py's compressor (then use --distinct 4); --reverse walks
compressors and routes backwards, so that two runs alternate the legs in both orders.
--content: `noise` = uniform random bytes (no codec shrinks them), `incompressible` = a smooth background plus Gaussian noise of sigma 6 (as tools/bench_loader.py; LZ4 does not shrink
it: Blosc stores its blocks raw), `compressible` = the same with the lower third of every frame a flat field (LZ4 shrinks it to
about two thirds).  --compressors: null, zlib (level 1), blosc (LZ4 blocks at --blocksize, framed here with the system's liblz4);
--decode: for blosc, zlib, blosc-zstd and zstd, `device` (yogo_blosc_lz4_decode / yogo_inflate_zlib / yogo_zstd_decode) and / or `host`
(ZarrDeviceFeed(device_decode=False)); the feed and the predict steps set zarr_feed.DEVICE_DECODE_ZLIB and DEVICE_DECODE_ZSTD from the
leg's route, whatever the module's defaults are.  Every measurement
is a step in a child process of its own with its own time limit; a step that fails or runs out of time is recorded as such, and
no further step is started.  The lines are APPENDED to --out.

  feed     ZarrDeviceFeed alone, batch 256, images/s on the host clock up to the final device synchronise (one warm-up pass,
           then the timed passes), (H, W, 1) chunks in a zip store of stored members
  decode   (blosc / zlib, device) yogo_blosc_lz4_decode / yogo_inflate_zlib alone on the first batch's rows, device events around
           each of 20 launches (zlib: 5), and the share of blocks stored raw
  predict  predict(count_predictions=True, half=True, device_outputs=True, batch_size=256), host clock around the whole call
  --unpack-kernel  yogo_zarr_unpack alone from device events, B = 256, against the bytes it has to move as a share of 8 TB/s
  --png            predict from the null store against the same frames as a PNG directory (16 workers), alternated

  python tools/bench_zarr_feed.py [--frames 1024] [--content incompressible,compressible] [--compressors null,zlib,blosc]
                                  [--decode device,host] [--out profiles/zarr_feed.log]
"""
import argparse
import ctypes
import ctypes.util
import json
import os
import shutil
import struct
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


def _frame(k: int, content: str = "incompressible") -> np.ndarray:
    rng = np.random.default_rng(k)
    if content == "noise":
        return rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    a, b, c = rng.uniform(0.5, 2.0, 3)
    smooth = 150 + 40 * np.sin(x / W * np.pi * a + c) * np.cos(y / H * np.pi * b)
    f = np.clip(smooth + rng.normal(0, 6, size=(H, W)), 0, 255).astype(np.uint8)
    if content == "compressible":
        f[2 * H // 3:] = int(f.mean())
    return f


def _lz4():
    name = ctypes.util.find_library("lz4")
    if not name:
        raise RuntimeError("the blosc stores of this tool are written with the system's liblz4, which is not installed")
    return ctypes.CDLL(name)


def blosc_lz4_frame(raw: bytes, blocksize: int) -> bytes:
    """one Blosc 1 chunk of uint8 data (yogo_amd/blosc.py describes the layout): LZ4 blocks, a block stored raw when LZ4 does not
    shrink it, the whole chunk memcpyed when the framing would make it longer than the data plus the header (as c-blosc does)"""
    L = _lz4()
    n = len(raw)
    nblocks = -(-n // blocksize)
    cap = L.LZ4_compressBound(blocksize)
    buf = ctypes.create_string_buffer(cap)
    body, bstarts, pos = bytearray(), [], 16 + 4 * nblocks
    for b in range(nblocks):
        block = raw[b * blocksize:(b + 1) * blocksize]
        got = L.LZ4_compress_default(block, buf, len(block), cap)
        enc = buf.raw[:got] if 0 < got < len(block) else block
        bstarts.append(pos)
        body += struct.pack("<i", len(enc)) + enc
        pos += 4 + len(enc)
    flags = 0x01 | (1 << 5)
    if pos > n + 16:
        return struct.pack("<BBBBIII", 2, 1, flags | 0x02, 1, n, blocksize, n + 16) + raw
    return struct.pack("<BBBBIII", 2, 1, flags, 1, n, blocksize, pos) + struct.pack(f"<{nblocks}i", *bstarts) + bytes(body)


ZSTD_LEVEL = 1
_zstd_cache: dict = {}


def zstd_writer() -> str:
    """what writes the Zstandard frames of the zstd legs: the system's libzstd through ctypes, or tests/_zstd_write.py's compressor"""
    from yogo_amd import zstd

    return f"libzstd {zstd.libzstd().ZSTD_versionString().decode()}" if zstd.libzstd() is not None else "tests/_zstd_write.py compress()"


def zstd_frame(raw: bytes) -> bytes:
    from yogo_amd import zstd

    if zstd.libzstd() is not None:
        return zstd.lib_compress(raw, ZSTD_LEVEL)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _zstd_write

    return _zstd_write.compress(raw)


def blosc_zstd_frame(raw: bytes, blocksize: int) -> bytes:
    """as blosc_lz4_frame with one Zstandard frame per block (inner format 4)"""
    n = len(raw)
    nblocks = -(-n // blocksize)
    body, bstarts, pos = bytearray(), [], 16 + 4 * nblocks
    for b in range(nblocks):
        block = raw[b * blocksize:(b + 1) * blocksize]
        enc = zstd_frame(block)
        if len(enc) >= len(block):
            enc = block
        bstarts.append(pos)
        body += struct.pack("<i", len(enc)) + enc
        pos += 4 + len(enc)
    flags = 0x01 | (4 << 5)
    if pos > n + 16:
        return struct.pack("<BBBBIII", 2, 1, flags | 0x02, 1, n, blocksize, n + 16) + raw
    return struct.pack("<BBBBIII", 2, 1, flags, 1, n, blocksize, pos) + struct.pack(f"<{nblocks}i", *bstarts) + bytes(body)


def _frames(d: str, n: int) -> np.ndarray:
    return np.memmap(os.path.join(d, "frames.u8"), dtype=np.uint8, mode="r", shape=(n, H, W))


def _gen(args):
    d, n, lo, hi, content, distinct = args
    m = np.memmap(os.path.join(d, "frames.u8"), dtype=np.uint8, mode="r+", shape=(n, H, W))
    for k in range(lo, hi):
        m[k] = _frame(k % distinct if distinct else k, content)
    m.flush()


def _png(args):
    from PIL import Image

    d, n, lo, hi = args
    m = _frames(d, n)
    for k in range(lo, hi):
        Image.fromarray(np.asarray(m[k]), mode="L").save(os.path.join(d, "png", f"img_{k:04d}.png"))


def _chunk(args):
    d, n, t, cn, compress, blocksize, distinct = args
    if distinct and cn == 1 and (compress, t % distinct) in _zstd_cache:   # (--distinct: frame t is frame t % distinct)
        return t, _zstd_cache[(compress, t % distinct)]
    m = _frames(d, n)
    block = np.zeros((H, W, cn), dtype=np.uint8)
    for j in range(cn):
        if t * cn + j < n:
            block[:, :, j] = m[t * cn + j]
    raw = block.tobytes()
    enc = ENCODERS[compress](raw, blocksize)
    if compress in ZSTD_WRITTEN and distinct and cn == 1:
        _zstd_cache[(compress, t % distinct)] = enc
    return t, enc


def _spans(n, parts):
    step = -(-n // parts)
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


ENCODERS = {"null": lambda raw, blocksize: raw, "zlib": lambda raw, blocksize: zlib.compress(raw, 1), "blosc": blosc_lz4_frame,
            "blosc-zstd": blosc_zstd_frame, "zstd": lambda raw, blocksize: zstd_frame(raw)}   # one chunk's bytes as the store holds them
ZSTD_WRITTEN = ("blosc-zstd", "zstd")   # the compressors whose frames zstd_writer() writes
COMPRESSOR_DOCS = {"null": None, "zlib": {"id": "zlib", "level": 1},
                   "blosc": {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0},
                   "blosc-zstd": {"id": "blosc", "cname": "zstd", "clevel": ZSTD_LEVEL, "shuffle": 1, "blocksize": 0},
                   "zstd": {"id": "zstd", "level": ZSTD_LEVEL}}


def write_store(d: str, n: int, name: str, cn: int, compress: str, blocksize: int = 131072, distinct: int = 0) -> str:
    """an [H, W, n] array in (H, W, cn) chunks as a zip store of stored members; compress: null, zlib, blosc, blosc-zstd or zstd"""
    p = os.path.join(d, name)
    meta = {"zarr_format": 2, "shape": [H, W, n], "chunks": [H, W, cn], "dtype": "|u1", "order": "C", "fill_value": 0, "filters": None,
            "compressor": COMPRESSOR_DOCS[compress], "dimension_separator": "."}
    with zipfile.ZipFile(p, "w", zipfile.ZIP_STORED) as zf, ProcessPoolExecutor(WORKERS) as ex:
        zf.writestr(".zarray", json.dumps(meta))
        for t, data in ex.map(_chunk, [(d, n, t, cn, compress, blocksize, distinct) for t in range(-(-n // cn))], chunksize=2):
            zf.writestr(f"0.0.{t}", data)
    return p


# ---- the steps (child processes) ------------------------------------------------------------------------------------------

def step_feed(store: str, n: int, device_decode: bool = True, passes: int = 2) -> dict:
    import torch

    from yogo_amd import zarr_feed
    from yogo_amd.image_path_dataset import ZarrDataset
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    # (the codecs whose device route is off by default: the leg's label decides, not the module's default)
    zarr_feed.DEVICE_DECODE_ZLIB = zarr_feed.DEVICE_DECODE_ZSTD = device_decode
    ds = ZarrDataset(store)
    rates, setup = [], []
    for p in range(passes + 1):
        t0 = time.perf_counter()
        feed = ZarrDeviceFeed(ds, B, "cuda", num_frames=n, device_decode=device_decode)   # allocates the pinned and the device buffers
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
    return {"images_per_s": rates, "setup_s": setup[1:], "bytes_on_disk": os.path.getsize(store), "last_pixel": acc,
            "device_decode": bool(feed.device_decode)}


def step_decode(store: str, n: int) -> dict:
    """the decode launches of the store's codec alone (zarr_feed.decode_rows, as the feed makes them: yogo_blosc_lz4_decode;
    yogo_inflate_zlib or yogo_zstd_decode with yogo_blosc_lz4_decode over the raw rows behind it) on the rows of the first batch"""
    import torch

    from yogo_amd.device_decode import zstd_work_bytes
    from yogo_amd.zarr_feed import CODECS, ChunkStager, FrameSource, decode_rows, plan_batch
    from yogo_amd.zarr_store import open_zarr

    src = FrameSource(open_zarr(store))
    codec = CODECS[src.first.device_codec]
    serial = not codec.copies_raw and not codec.workspace   # (one wavefront per chunk and no more: the launches are long)
    launches = 5 if serial else 20
    plan = plan_batch(src, 0, min(B, n))
    stager = ChunkStager(src)
    buf = np.zeros(len(plan.keys) * src.stored_stride, np.uint8)
    try:
        table = stager.stage_stored(plan, buf)
    finally:
        stager.close()
    raw = plan.row_raw
    stored = torch.from_numpy(buf).cuda()
    table_dev = torch.from_numpy(table).cuda()
    out = torch.empty(plan.nbytes, dtype=torch.uint8, device="cuda")
    status = torch.empty(len(table), dtype=torch.int32, device="cuda")
    work = torch.empty(zstd_work_bytes(max(len(raw) - int(raw.sum()), 1)), dtype=torch.uint8, device="cuda") if codec.workspace else None
    for _ in range(1 if serial else 3):
        decode_rows(codec, stored, table_dev, raw, out, status, work)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    ev[0].record()
    for i in range(launches):
        decode_rows(codec, stored, table_dev, raw, out, status, work)
        ev[i + 1].record()
    torch.cuda.synchronize()
    us = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(launches))
    return {"median_us": us[launches // 2], "min_us": us[0], "blocks": int(len(table)), "raw_blocks": int(raw.sum()),
            "stored_bytes": int(table[:, 1].sum()), "decoded_bytes": int(table[:, 3].sum()), "all_ok": not bool(status.any()),
            "frames": int(plan.hi - plan.lo)}


def step_kernel() -> list:
    import torch

    from yogo_amd import _hip
    from yogo_amd.device_decode import ALIGN
    from yogo_amd.zarr_feed import unpack

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


def step_predict_store(d: str, store: str, n: int, route: str = "device") -> dict:
    """predict --count --device-outputs from one store, twice; route host: a zlib store is inflated on the host"""
    import contextlib
    import io

    import torch

    from yogo_amd import zarr_feed
    from yogo_amd.infer import predict
    from yogo_amd.model import YOGO

    zarr_feed.DEVICE_DECODE_ZLIB = zarr_feed.DEVICE_DECODE_ZSTD = route == "device"

    torch.manual_seed(3)
    net = YOGO((H, W), 0.0425, 0.0555, 4).cuda().eval()
    pth = os.path.join(d, "m.pth")
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "bench",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, pth)
    del net
    res = {"s": [], "counts": []}
    for rep in range(2):
        buf = io.StringIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(buf):
            predict(pth, path_to_zarr=store, count_predictions=True, half=True, batch_size=B, class_names=CLASSES, device_outputs=True)
        torch.cuda.synchronize()
        res["s"].append(time.perf_counter() - t0)
        res["counts"].append(buf.getvalue().strip().splitlines()[-1])
    res["counts"] = res["counts"][0] if len(set(res["counts"])) == 1 else res["counts"]
    return res


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
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--content", default="incompressible,compressible")
    ap.add_argument("--compressors", default="null,zlib,blosc")
    ap.add_argument("--decode", default="device,host", help="for blosc and zlib stores: device and / or host")
    ap.add_argument("--blocksize", type=int, default=131072, help="Blosc block size (c-blosc's choice for 1-byte items at clevel 5)")
    ap.add_argument("--distinct", type=int, default=0, help="K > 0: frame k is frame k % K (a slow writer then compresses K frames only)")
    ap.add_argument("--reverse", action="store_true", help="walk the compressors and the routes in reverse order (the second half of an alternated run)")
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--unpack-kernel", action="store_true")
    ap.add_argument("--png", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zarr_feed.log"))
    ap.add_argument("--step", default=None)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    if a.step:
        if a.step == "feed":
            res = step_feed(a.rest[0], int(a.rest[1]), a.rest[2] == "device")
        elif a.step == "decode":
            res = step_decode(a.rest[0], int(a.rest[1]))
        elif a.step == "kernel":
            res = step_kernel()
        elif a.step == "predict_store":
            res = step_predict_store(a.rest[0], a.rest[1], int(a.rest[2]), *a.rest[3:4])
        else:
            res = step_predict(a.rest[0], a.rest[1], int(a.rest[2]))
        print("RESULT " + json.dumps(res), flush=True)
        return 0

    n = a.frames

    def log(s=""):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    d = tempfile.mkdtemp(prefix="zarr_bench_")
    try:
        log()
        log(f"tools/bench_zarr_feed.py --frames {n} --content {a.content} --compressors {a.compressors} --decode {a.decode} "
            f"--blocksize {a.blocksize} on one MI355X ({time.strftime('%Y-%m-%d')}); seeded {H}x{W} uint8 frames, batch {B}, (H, W, 1) chunks, "
            "zip stores written just before (reads come from the page cache, not from a disk)")
        log("feed = ZarrDeviceFeed alone, images/s on the host clock, timed passes after a warm-up pass; predict = predict(count_predictions, "
            "half, device_outputs), host clock around the whole call (model load included); decode = the device decoder alone on the first "
            "batch, device events, median / min of 20 launches (zlib: 5)")
        if any(c in ZSTD_WRITTEN for c in a.compressors.split(",")):
            log(f"Zstandard frames written by {zstd_writer()} at level {ZSTD_LEVEL}; Blosc-zstd: one frame per block of {a.blocksize} bytes, a block stored "
                f"raw when its frame is no shorter; --distinct {a.distinct}" + ("; compressors and routes walked in REVERSE order" if a.reverse else ""))
        ok = True
        for content in a.content.split(","):
            np.memmap(os.path.join(d, "frames.u8"), dtype=np.uint8, mode="w+", shape=(n, H, W)).flush()
            with ProcessPoolExecutor(WORKERS) as ex:
                list(ex.map(_gen, [(d, n, lo, hi, content, a.distinct) for lo, hi in _spans(n, WORKERS * 4)]))
            log(f"content {content}:")
            for comp in (a.compressors.split(",")[::-1] if a.reverse else a.compressors.split(",")):
                store = write_store(d, n, f"{content}_{comp}.zip", 1, comp, a.blocksize, a.distinct)
                share = os.path.getsize(store) / n / (H * W) * 100
                routed = comp in ("blosc", "zlib", "blosc-zstd", "zstd")
                for route in ((a.decode.split(",")[::-1] if a.reverse else a.decode.split(",")) if routed else ["host"]):
                    label = f"  {comp:<10s} {('decode on the ' + route) if routed else '':<20s}"
                    r = run_step(log, "feed", 300, [store, n, route])
                    if r is None:
                        ok = False
                        break
                    log(f"{label} feed     " + "  ".join(f"{v:9.0f} img/s" for v in r["images_per_s"]) +
                        f"   ({share:.1f} % of raw on disk; device_decode={r['device_decode']})")
                    if routed and route == "device":
                        k = run_step(log, "decode", 180, [store, n])
                        if k is None:
                            ok = False
                            break
                        log(f"{label} decode   {k['median_us']:9.1f} us / {k['min_us']:9.1f} us per batch of {k['frames']} frames: {k['blocks']} blocks, "
                            f"{k['raw_blocks']} of them raw ({100 * k['raw_blocks'] / max(k['blocks'], 1):.1f} %), {k['stored_bytes'] / 1e6:.1f} MB stored -> "
                            f"{k['decoded_bytes'] / 1e6:.1f} MB decoded = {k['decoded_bytes'] / (k['median_us'] * 1e-6) / 1e9:.0f} GB/s out; every status 0: {k['all_ok']}")
                    if not a.no_predict and (comp not in ("blosc", "blosc-zstd") or route == "device"):
                        r = run_step(log, "predict_store", 420, [d, store, n, route])
                        if r is None:
                            ok = False
                            break
                        log(f"{label} predict  " + "  ".join(f"{t:7.2f} s = {n / t:8.0f} img/s" for t in r["s"]) + f"   {r['counts']}")
                if comp != "null" or not a.png or not ok:
                    os.remove(store)
                if not ok:
                    break
            if not ok:
                break
            if a.png:
                raw_store = os.path.join(d, f"{content}_null.zip")
                if os.path.exists(raw_store):
                    os.makedirs(os.path.join(d, "png"), exist_ok=True)
                    with ProcessPoolExecutor(WORKERS) as ex:
                        list(ex.map(_png, [(d, n, lo, hi) for lo, hi in _spans(n, WORKERS * 4)]))
                    r = run_step(log, "predict", 420, [d, raw_store, n])
                    if r is not None:
                        for kind, label in (("zarr", "(H, W, 1) raw zip"), ("png", "PNG directory    ")):
                            log(f"  predict(count_predictions, half), alternated: {label}  " + "  ".join(f"{t:7.2f} s = {n / t:8.0f} img/s" for t in r[kind + "_s"]))
                        log(f"  the four runs print the same counts: {r['same_counts']}   {r['counts']}")
                    os.remove(raw_store)
        if ok and a.unpack_kernel:
            log(f"yogo_zarr_unpack alone, B = {B}, device events around each of 20 launches (median / min), bytes = frames read + output written")
            for k in run_step(log, "kernel", 180, []) or []:
                log(f"  {k['kernel']:<42s} cn={k['cn']:<3d} {k['median_us']:8.1f} us / {k['min_us']:8.1f} us   {k['bytes_moved'] / 1e6:7.1f} MB   "
                    f"{k['bytes_moved'] / (k['median_us'] * 1e-6) / 1e12:5.2f} TB/s = {k['share_of_8TBps'] * 100:4.1f} % of 8 TB/s"
                    f"   equals the host's slicing: {k['matches_host']}")
        return 0 if ok else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
