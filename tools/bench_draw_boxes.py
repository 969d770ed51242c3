"""`predict --draw-boxes` on the host route (PIL, image by image) and on the device route (``device_draw=True``: yogo_amd/draw.py), one
process, one GPU.

--frames frames of 772 x 1032 (default 1024; --distinct distinct ones, smooth background, dark cells, sensor noise) in a raw zarr
directory stack, read once beforehand so that it sits in the page cache; batch 256; a random-init base_model (7 classes) with the
objectness threshold bisected on the network's own output until threshold + NMS keeps 96 boxes per image of the first 16 frames (the log states what a whole batch keeps), the firing rate README.md quotes.
The routes run in the order host, device, device, host (so each runs first and last once) and are reported per pass:

  images/s of predict(draw_boxes=True, output_dir=...) per route, wall clock around the call (model load and atlas build included)
  per launch: the render kernel and the encode call (two launches), HIP events around them on a batch of the run's own frames
  the read-back (offsets, then the file bytes) and the file writes (the pool of at most 8 threads) of one batch, host clock
  mean file size: the device route's files, PIL's compress_level=1 files of the same pixels (the host route's), the stored size

The tool checks on --check files that both routes decode to the same pixels, and asserts no ratio.  It needs the GPU.

--level is another leg, the device route alone at the PNG encoder's two levels (``device_draw_level``: 0 literals only, 1 literals
and LZ77 matches), one process: the route in the order 0, 1, 1, 0, and per level on one batch of the run's own drawn frames the
encode call, the read-back (bytes and time), the file writes and the bytes per file beside PIL's compress_level=1 for the same
pixels; the levels' launches alternate trip by trip.  --parent-lib PATH adds level 0's encode call through another build of the
library (the parent commit's), alternated with this build's on the same frames: what "level 0 did not slow down" is read from.

  python tools/bench_draw_boxes.py [--frames 1024] [--out profiles/draw_boxes.log]
  python tools/bench_draw_boxes.py --level [--parent-lib DIR/libyogo_hip.so] [--out profiles/draw_boxes_matches.log]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, C, BOXES = 772, 1032, 7, 96
CLASSES = ["healthy", "ring", "trophozoite", "schizont", "gametocyte", "wbc", "misc"]


def make_frames(n: int, seed: int = 0) -> np.ndarray:
    """[n, H, W] uint8: a smooth bright field, a few hundred dark round cells, Gaussian noise of sigma 2"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W), dtype=np.uint8)
    for k in range(n):
        f = 190 + 20 * np.cos(xx / W * rng.uniform(1, 3) + rng.uniform(0, 6)) * np.cos(yy / H * rng.uniform(1, 3) + rng.uniform(0, 6))
        for _ in range(200):
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(12, 22)
            x0, x1, y0, y1 = int(max(cx - r, 0)), int(min(cx + r + 1, W)), int(max(cy - r, 0)), int(min(cy + r + 1, H))
            d = np.hypot(xx[y0:y1, x0:x1] - cx, yy[y0:y1, x0:x1] - cy)
            f[y0:y1, x0:x1] -= 60 * np.clip(r - d, 0, 3) / 3
        out[k] = np.clip(f + rng.normal(0, 2, (H, W)), 0, 255).astype(np.uint8)
    return out


def write_raw_stack(path: str, frames: np.ndarray, n: int) -> str:
    """a zarr v2 directory store, array [H, W, n] of uint8, one uncompressed chunk per frame (frame k is frames[k % len(frames)])"""
    os.makedirs(path)
    with open(os.path.join(path, ".zarray"), "w") as f:
        json.dump({"zarr_format": 2, "shape": [H, W, n], "chunks": [H, W, 1], "dtype": "|u1", "compressor": None, "fill_value": 0,
                   "order": "C", "filters": None}, f)
    for k in range(n):
        with open(os.path.join(path, f"0.0.{k}"), "wb") as f:
            f.write(frames[k % len(frames)].tobytes())
    return path


def make_checkpoint(path: str) -> str:
    from yogo_amd.model import YOGO

    torch.manual_seed(0)
    net = YOGO((H, W), 0.0425, 0.0555, C).cuda().eval()
    with torch.no_grad():   # trained-like running statistics keep the eval-mode activations in range (as the tests' checkpoints)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 50.0)
                m.running_var.uniform_(2000.0, 9000.0)
    torch.save({"epoch": 0, "step": 0, "normalize_images": False, "classes": CLASSES, "model_name": "bench",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, path)
    return path


def threshold_for(pth: str, frames: np.ndarray) -> float:
    """the objectness threshold at which threshold + NMS keeps BOXES boxes per image, by bisection on the network's own output for
    the first frames (a random-init network fires in clusters that NMS thins out, so the count of firing cells is not the count kept)"""
    from yogo_amd.model import YOGO
    from yogo_amd.utils.prediction_formatting import format_preds_batched

    net, _ = YOGO.from_pth(pth, inference=True)
    net.eval().cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        dec = net(torch.from_numpy(frames[:16, None]).cuda()).float()
    lo, hi = 0.0, 1.0   # kept boxes fall as the threshold rises
    for _ in range(24):
        mid = (lo + hi) / 2
        kept = float(format_preds_batched(dec, mid, 0.5, "xyxy", 0.0)[2].float().mean())
        if kept > BOXES:
            lo = mid
        else:
            hi = mid
    return hi


def level_leg(args, say, tmp: str, frames: np.ndarray, stack: str, pth: str, thresh: float) -> None:
    """the device route at the encoder's levels 0 and 1 (the module's docstring)"""
    import ctypes
    import io
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    from yogo_amd import _hip, draw
    from yogo_amd.infer import predict
    from yogo_amd.model import YOGO
    from yogo_amd.utils.prediction_formatting import format_preds_batched

    kw = dict(path_to_zarr=stack, draw_boxes=True, batch_size=args.batch_size, obj_thresh=thresh, class_names=CLASSES, half=True,
              device_draw=True)
    rates, dirs = {0: [], 1: []}, {}
    for n_pass, level in enumerate((0, 1, 1, 0)):
        out = os.path.join(tmp, f"level{level}_{n_pass}")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        predict(pth, output_dir=out, device_draw_level=level, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates[level].append(args.frames / dt)
        say(f"  pass {n_pass} level {level}: {dt:8.2f} s   {args.frames / dt:9.1f} images/s   ({dt / args.frames * 1e3:7.2f} ms per image)")
        if level in dirs:
            shutil.rmtree(out)
        else:
            dirs[level] = out
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and len(names) == args.frames
    sample = names[:: max(1, len(names) // args.check)]
    pil_bytes, same = [], True
    for f in sample:
        a, b = np.asarray(Image.open(os.path.join(dirs[0], f))), np.asarray(Image.open(os.path.join(dirs[1], f)))
        same = same and np.array_equal(a, b)
        buf = io.BytesIO()
        Image.fromarray(a, mode="RGBA").save(buf, format="PNG", compress_level=1)
        pil_bytes.append(len(buf.getvalue()))
    size = {lv: float(np.mean([os.path.getsize(os.path.join(dirs[lv], f)) for f in names])) for lv in dirs}
    sampled = {lv: float(np.mean([os.path.getsize(os.path.join(dirs[lv], f)) for f in sample])) for lv in dirs}
    pil = float(np.mean(pil_bytes))
    say(f"  both levels wrote the same {len(names)} file names; {len(sample)} sampled files decode to the same pixels: {'yes' if same else 'NO'}")
    say(f"  mean file size over all files: level 0 {size[0] / 1e6:.3f} MB, level 1 {size[1] / 1e6:.3f} MB   level 1 / level 0 = {size[1] / size[0]:.3f}")
    say(f"  over the {len(sample)} sampled files: level 0 {sampled[0] / 1e6:.3f} MB, level 1 {sampled[1] / 1e6:.3f} MB, PIL compress_level=1 "
        f"{pil / 1e6:.3f} MB   level 0 / PIL = {sampled[0] / pil:.2f}, level 1 / PIL = {sampled[1] / pil:.2f}")

    net, _ = YOGO.from_pth(pth, inference=True)
    net.eval().cuda()
    B = min(args.batch_size, args.frames)
    x = torch.from_numpy(np.stack([frames[k % len(frames)] for k in range(B)])[:, None]).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        rows, _, counts = format_preds_batched(net.forward_raw(x), thresh, 0.5, "xyxy", 0.0)
    atlas = draw.DeviceAtlas(draw.GlyphAtlas(CLASSES), 1, "cuda")
    rgba = draw.render_boxes(x, rows, counts, atlas, False)
    slot, work0 = draw.encode_bound(H, W, 4, level=0)
    _, work1 = draw.encode_bound(H, W, 4, level=1)
    files = torch.empty(B * slot, dtype=torch.uint8, device="cuda")
    work = torch.empty(B * work1, dtype=torch.uint8, device="cuda")
    say(f"  one batch of {B}: {float(counts.float().mean()):.1f} boxes per image; buffers: RGBA frames {rgba.numel() / 1e9:.2f} GB, file slots "
        f"{files.numel() / 1e9:.2f} GB, encoder work space {B * work0 / 1e9:.2f} GB at level 0 and {B * work1 / 1e9:.2f} GB at level 1")

    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    offsets = torch.empty(B + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")

    this = _hip.lib()
    for L in (this, parent):   # the same direct call for every leg: no wrapper's host work between the events
        if L is not None:
            L.yogo_png_encode.restype = ctypes.c_int
            L.yogo_png_encode.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] +
                                          [ctypes.c_void_p] * 3 + [ctypes.c_longlong, ctypes.c_void_p])

    def encode(which):
        tail = (files.data_ptr(), slot, 1, offsets.data_ptr(), status.data_ptr(), work.data_ptr())
        if which == 1:
            rc = this.yogo_png_encode_level(rgba.data_ptr(), B, H, W, 4, 1, *tail, B * work1, _hip.stream_ptr())
        else:
            rc = (parent if which == "parent" else this).yogo_png_encode(rgba.data_ptr(), B, H, W, 4, *tail, B * work0, _hip.stream_ptr())
        assert rc == 0
        return offsets, status

    legs = ([("parent", "level 0, the other build")] if parent is not None else []) + [(0, "level 0"), (1, "level 1")]
    t = {which: dict(encode=[], read=[], write=[], bytes=0) for which, _ in legs}
    for it in range(args.trips + 1):
        for which, _ in legs[it % len(legs):] + legs[: it % len(legs)]:   # alternated: each once per trip, the first one rotating
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            off_d, st_d = encode(which)
            ev[1].record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            off = off_d.cpu().numpy()
            data = files[: int(off[B])].cpu().numpy()
            t1 = time.perf_counter()
            view = memoryview(data)
            with ThreadPoolExecutor(max_workers=draw.MAX_WRITERS) as pool:
                list(pool.map(lambda k: draw._write(os.path.join(tmp, f"w_{k}.png"), view[int(off[k]): int(off[k + 1])]), range(B)))
            t2 = time.perf_counter()
            assert int(st_d.abs().sum()) == 0
            if it:   # the first trip is a warm-up
                t[which]["encode"].append(ev[0].elapsed_time(ev[1]))
                t[which]["read"].append((t1 - t0) * 1e3)
                t[which]["write"].append((t2 - t1) * 1e3)
            t[which]["bytes"] = int(off[B])
    for which, label in legs:
        say(f"  {label}: {t[which]['bytes'] / B / 1e6:.3f} MB per file, read back {t[which]['bytes'] / 1e6:.1f} MB per batch of {B}")
        for name, key in (("encode (two launches)", "encode"), ("read-back", "read"), ("file writes", "write")):
            v = t[which][key]
            say(f"    {name:22s} ms: " + " ".join(f"{u:8.2f}" for u in v) + f"   median {np.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
    say()
    say(f"predict --draw-boxes --device-draw: level 0 {' / '.join(f'{v:.1f}' for v in rates[0])} images/s, level 1 "
        f"{' / '.join(f'{v:.1f}' for v in rates[1])} images/s   level 1 / level 0 = {np.median(rates[1]) / np.median(rates[0]):.2f}x")
    say("level 1 faster than level 0 in both orders: " + ("yes" if min(rates[1]) > max(rates[0]) else "NO"))
    say(f"level 1's files smaller than level 0's: {'yes' if size[1] < size[0] else 'NO'}; smaller than PIL's compress_level=1 files: "
        f"{'yes' if sampled[1] < pil else 'NO'}")
    if parent is not None:
        p, c = t["parent"]["encode"], t[0]["encode"]
        say(f"level 0's encode call, this build against the other: median {np.median(c):.2f} ms against {np.median(p):.2f} ms; the other "
            f"build's own repeats span {min(p):.2f} .. {max(p):.2f} ms; inside that span or below it: {'yes' if np.median(c) <= max(p) else 'NO'}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--check", type=int, default=8, help="files compared pixel for pixel between the routes")
    ap.add_argument("--level", action="store_true", help="the device route at the PNG encoder's levels 0 and 1 instead of host against device")
    ap.add_argument("--parent-lib", default=None, help="with --level: another build of libyogo_hip.so whose level-0 encode call is timed beside this one's")
    ap.add_argument("--trips", type=int, default=7, help="with --level: timed trips per build and level (one more warms up)")
    ap.add_argument("--out", default=None, help="default: profiles/draw_boxes.log, with --level profiles/draw_boxes_matches.log")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "draw_boxes_matches.log" if args.level else "draw_boxes.log")
    if args.parent_lib and not args.level:
        ap.error("--parent-lib belongs to the --level leg")
    if not torch.cuda.is_available():
        print("tools/bench_draw_boxes.py needs the MI355X: there is no fallback and nothing to report without it", file=sys.stderr)
        return 2
    from PIL import Image

    from yogo_amd import draw
    from yogo_amd.infer import predict
    from yogo_amd.utils.prediction_formatting import format_preds_batched

    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = []

    def say(text: str = "") -> None:
        print(text, flush=True)
        lines.append(text)

    tmp = tempfile.mkdtemp(prefix="draw_boxes_")
    try:
        frames = make_frames(args.distinct)
        stack = write_raw_stack(os.path.join(tmp, "stack.zarr"), frames, args.frames)
        for k in range(args.frames):   # into the page cache
            with open(os.path.join(stack, f"0.0.{k}"), "rb") as f:
                f.read()
        pth = make_checkpoint(os.path.join(tmp, "m.pth"))
        thresh = threshold_for(pth, frames)
        if args.level:
            say(f"tools/bench_draw_boxes.py --level on one MI355X: {args.frames} frames of {H} x {W} ({args.distinct} distinct) from a raw zarr "
                f"stack in the page cache, batch {args.batch_size}, random-init base_model, {C} classes, obj_thresh {thresh:.6f} (about {BOXES} "
                f"boxes per image), bf16 forward, torch threads {torch.get_num_threads()}, at most {draw.MAX_WRITERS} writer threads")
            level_leg(args, say, tmp, frames, stack, pth, thresh)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
            return 0
        say(f"tools/bench_draw_boxes.py on one MI355X: {args.frames} frames of {H} x {W} ({args.distinct} distinct) from a raw zarr stack in the "
            f"page cache, batch {args.batch_size}, random-init base_model, {C} classes, obj_thresh {thresh:.6f} (about {BOXES} boxes per image), "
            f"bf16 forward, torch threads {torch.get_num_threads()}, at most {draw.MAX_WRITERS} writer threads")
        kw = dict(path_to_zarr=stack, draw_boxes=True, batch_size=args.batch_size, obj_thresh=thresh, class_names=CLASSES, half=True)
        rates = {"host": [], "device": []}
        dirs = {}
        for n_pass, route in enumerate(("host", "device", "device", "host")):
            out = os.path.join(tmp, f"{route}_{n_pass}")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            predict(pth, output_dir=out, device_draw=route == "device", **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rates[route].append(args.frames / dt)
            say(f"  pass {n_pass} {route:6s} route: {dt:8.2f} s   {args.frames / dt:9.1f} images/s   ({dt / args.frames * 1e3:7.2f} ms per image)")
            if route in dirs:
                shutil.rmtree(out)
            else:
                dirs[route] = out
        names = sorted(os.listdir(dirs["host"]))
        assert names == sorted(os.listdir(dirs["device"])) and len(names) == args.frames
        same = all(np.array_equal(np.asarray(Image.open(os.path.join(dirs["host"], f))), np.asarray(Image.open(os.path.join(dirs["device"], f))))
                   for f in names[:: max(1, len(names) // args.check)])
        say(f"  the routes wrote the same {len(names)} file names; sampled files decode to the same pixels: {'yes' if same else 'NO'}")
        size = {r: float(np.mean([os.path.getsize(os.path.join(dirs[r], f)) for f in names])) for r in dirs}
        stored = draw.encode_bound(H, W, 4)[0]
        say(f"  mean file size: device route {size['device'] / 1e6:.3f} MB, PIL compress_level=1 (host route) {size['host'] / 1e6:.3f} MB, "
            f"stored {stored / 1e6:.3f} MB   device / PIL = {size['device'] / size['host']:.2f}, device / stored = {size['device'] / stored:.2f}")

        # the launches and the host work of one batch of the device route
        from yogo_amd.model import YOGO

        net, _ = YOGO.from_pth(pth, inference=True)
        net.eval().cuda()
        B = min(args.batch_size, args.frames)
        x = torch.from_numpy(np.stack([frames[k % len(frames)] for k in range(B)])[:, None]).cuda()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            rows, _, counts = format_preds_batched(net.forward_raw(x), thresh, 0.5, "xyxy", 0.0)
        say(f"  one batch of {B}: {float(counts.float().mean()):.1f} boxes per image (min {int(counts.min())}, max {int(counts.max())})")
        atlas = draw.DeviceAtlas(draw.GlyphAtlas(CLASSES), 1, "cuda")
        slot, work_per = draw.encode_bound(H, W, 4)
        rgba = torch.empty(B, H, W, 4, dtype=torch.uint8, device="cuda")
        files = torch.empty(B * slot, dtype=torch.uint8, device="cuda")
        work = torch.empty(B * work_per, dtype=torch.uint8, device="cuda")
        say(f"  buffers for a batch of {B}: RGBA frames {rgba.numel() / 1e9:.2f} GB, file slots {files.numel() / 1e9:.2f} GB, "
            f"encoder work space {work.numel() / 1e9:.2f} GB")
        t_render, t_encode, t_read, t_write = [], [], [], []
        for it in range(6):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            draw.render_boxes(x, rows, counts, atlas, False, out=rgba)
            ev[1].record()
            _, offsets, status = draw.encode_png(rgba, files, work, packed=True)
            ev[2].record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            off = offsets.cpu().numpy()
            data = files[: int(off[B])].cpu().numpy()
            t1 = time.perf_counter()
            view = memoryview(data)
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max_workers=draw.MAX_WRITERS) as pool:
                list(pool.map(lambda k: draw._write(os.path.join(tmp, f"w_{k}.png"), view[int(off[k]): int(off[k + 1])]), range(B)))
            t2 = time.perf_counter()
            if it:   # the first trip is a warm-up
                t_render.append(ev[0].elapsed_time(ev[1]))
                t_encode.append(ev[1].elapsed_time(ev[2]))
                t_read.append((t1 - t0) * 1e3)
                t_write.append((t2 - t1) * 1e3)
            assert int(status.abs().sum()) == 0
        for name, v in (("render launch", t_render), ("encode (two launches)", t_encode), ("read-back", t_read), ("file writes", t_write)):
            say(f"  {name:22s} per batch of {B}, ms: " + " ".join(f"{t:8.2f}" for t in v) + f"   median {np.median(v):8.2f}"
                f"   ({np.median(v) / B * 1e3:7.1f} us per image)")
        say(f"  read back per batch: {int(off[B]) / 1e6:.1f} MB")
        say()
        mh, md = float(np.median(rates["host"])), float(np.median(rates["device"]))
        say(f"predict --draw-boxes: host route {' / '.join(f'{v:.1f}' for v in rates['host'])} images/s, device route "
            f"{' / '.join(f'{v:.1f}' for v in rates['device'])} images/s   device / host = {md / mh:.1f}x")
        say("device route faster than the host route in both orders: " + ("yes" if min(rates["device"]) > max(rates["host"]) else "NO"))
        say("device route's files smaller than PIL's compress_level=1 files: " + ("yes" if size["device"] < size["host"] else "NO"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
