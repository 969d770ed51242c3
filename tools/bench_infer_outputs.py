"""Seconds per batch of `yogo infer`'s output stage -- everything from the threshold + NMS launch to the host results -- on the default
host path and on the sink path (``predict(..., device_outputs=True)``, yogo_amd/pred_sink.py), one process, one GPU.

Decoded predictions at the production geometry ([B, 12, 97, 129]: 772 x 1032 images, 7 classes), B = 64 (the CLI default) and
B = 256, about 96 firing cells per image, built on the device from a seed.  For each of the three outputs:

  count   get_prediction_class_counts                          | format_preds_batched + PredictionSink.add_counts, class_counts() at the end
  npy     format_to_numpy_batched                              | format_preds_batched + PredictionSink.append, one drain() at the end
  preds   save_predictions (text formatting and file writes)   | format_preds_batched + append, one drain(), the same formatting and writes
                                                               | text path: format_preds_batched + append, one drain_text() -- the text is
                                                               |   formatted on the device (yogo_amd/csrc/pred_text.hip) -- and the writes

A round runs the host path over --batches batches and then the sink path over the same batches with its final read-out inside the timed
window (so the drain is amortised over the batches); rounds alternate the two paths, the first round is a warm-up, and the host clock
stops after a device synchronise.  The host path's code is what every earlier version runs.  For preds a third path alternates with
the two in the same rounds: the text path, which is what `predict(save_preds=True, device_outputs=True)` runs; the sink path's row
stays the host formatting of the drained records, as shipped before the device formatter.  The tool checks that the paths
gave the same results, reports seconds per batch of every round and the bytes each path copies to the host per batch, and asserts no
ratio.  It needs the GPU: there is no fallback.

  python tools/bench_infer_outputs.py [--out profiles/infer_outputs.log] [--append]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

C, SY, SX, K = 7, 97, 129, 96
IMG_H, IMG_W = 772, 1032


def make_preds(B: int, seed: int) -> torch.Tensor:
    """decoded predictions with K firing cells per image: small boxes on their cells (NMS keeps nearly all), objectness 0.6 .. 1 on
    them and 0.05 elsewhere, class scores a softmax of 3 * randn"""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    p = torch.empty(B, 5 + C, SY, SX, device=dev)
    ys = (torch.arange(SY, device=dev, dtype=torch.float32) + 0.5) / SY
    xs = (torch.arange(SX, device=dev, dtype=torch.float32) + 0.5) / SX
    p[:, 0] = xs[None, None, :]
    p[:, 1] = ys[None, :, None]
    p[:, 2] = 0.5 / SX
    p[:, 3] = 0.5 / SY
    fire = torch.rand(B, SY * SX, device=dev, generator=g).argsort(1)[:, :K]
    obj = torch.full((B, SY * SX), 0.05, device=dev)
    obj.scatter_(1, fire, 0.6 + 0.4 * torch.rand(B, K, device=dev, generator=g))
    p[:, 4] = obj.view(B, SY, SX)
    p[:, 5:] = (3 * torch.randn(B, C, SY, SX, device=dev, generator=g)).softmax(1)
    return p


class Legs:
    """the two paths of one output for one batch size; ``host(batches)`` / ``sink(batches)`` run a round and return its results"""

    def __init__(self, kind: str, B: int, tmp: str):
        from yogo_amd.pred_sink import PredictionSink

        self.kind, self.B, self.tmp = kind, B, tmp
        dev = torch.device("cuda")
        self.snk = PredictionSink(dev, C, "npy", img_hw=(IMG_H, IMG_W)) if kind == "npy" else PredictionSink(dev, C, "rows")
        self.txt_snk = PredictionSink(dev, C, "rows") if kind == "preds" else None
        self.host_bytes = 0.0   # per batch, from the shapes of what .cpu() is called on
        self.sink_bytes = 0.0
        self.text_bytes = 0.0
        self.write_ms = []      # per round of the text path: its file writes alone, per batch

    def names(self, tag: str, n_batches: int):
        return [[os.path.join(self.tmp, f"{tag}_{i}_{j}.txt") for j in range(self.B)] for i in range(n_batches)]

    def host(self, batches):
        from yogo_amd.utils import format_to_numpy_batched, get_prediction_class_counts, save_predictions

        B, cap, P = self.B, SY * SX, 5 + C
        if self.kind == "count":
            tot = torch.zeros(C)
            for p in batches:
                tot += get_prediction_class_counts(p, obj_thresh=0.5, iou_thresh=0.5, min_class_confidence_threshold=0.0)
            self.host_bytes = B * 4 + B * C * 8      # the counts, then one class histogram per image (B synchronisations)
            return [int(v) for v in tot]
        if self.kind == "npy":
            out = []
            for i, p in enumerate(batches):
                out.extend(format_to_numpy_batched([i * B + j for j in range(B)], p, IMG_H, IMG_W))
            self.host_bytes = B * cap * P * 4 + B * 4
            return np.hstack(out)
        names = self.names("host", len(batches))
        for p, fn in zip(batches, names):
            save_predictions(fn, p, obj_thresh=0.5, iou_thresh=0.5)
        self.host_bytes = B * cap * P * 4 + B * 4
        return names

    def sink(self, batches):
        from yogo_amd.pred_sink import npy_columns, split_records
        from yogo_amd.utils.prediction_formatting import format_preds_batched, prediction_rows_to_text

        B, s = self.B, self.snk
        if self.kind == "count":
            before = s.class_counts()
            for p in batches:
                rows, _, counts = format_preds_batched(p, 0.5, 0.5, "cxcywh", 0.0)
                s.add_counts(rows, counts)
            self.sink_bytes = 2 * C * 8 / len(batches)
            return [int(v) for v in s.class_counts() - before]
        if self.kind == "npy":
            for i, p in enumerate(batches):
                rows, _, counts = format_preds_batched(p, box_format="xyxy")
                s.append(rows, counts, i * B)
            rec, per = s.drain()
            self.sink_bytes = (rec.nbytes + per.nbytes + 4 * 8) / len(batches)
            return npy_columns([(rec, per)], C)
        names = self.names("sink", len(batches))
        for i, p in enumerate(batches):
            rows, _, counts = format_preds_batched(p, 0.5, 0.5)
            s.append(rows, counts, i * B)
        rec, per = s.drain()
        self.sink_bytes = (rec.nbytes + per.nbytes + 4 * 8) / len(batches)
        flat = [f for fn in names for f in fn]
        for fname, r in zip(flat, split_records(rec, per)):
            with open(fname, "w") as f:
                f.write(prediction_rows_to_text(torch.from_numpy(r)))
        return names

    def text(self, batches):
        """preds only: the text comes formatted from the device, the host writes byte ranges"""
        from yogo_amd.utils.prediction_formatting import format_preds_batched

        B, s = self.B, self.txt_snk
        names = self.names("text", len(batches))
        for i, p in enumerate(batches):
            rows, _, counts = format_preds_batched(p, 0.5, 0.5)
            s.append(rows, counts, i * B)
        text, offsets = s.drain_text()
        self.text_bytes = (text.nbytes + offsets.nbytes + 8 + 4 * 8) / len(batches)
        data = memoryview(text)
        t0 = time.perf_counter()
        for k, fname in enumerate(f for fn in names for f in fn):
            with open(fname, "wb") as f:
                f.write(data[offsets[k]: offsets[k + 1]])
        self.write_ms.append((time.perf_counter() - t0) * 1e3 / len(batches))
        return names

    def same(self, a, b) -> bool:
        if self.kind == "count":
            return a == b
        if self.kind == "npy":
            return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
        return all(open(x, "rb").read() == open(y, "rb").read() for fa, fb in zip(a, b) for x, y in zip(fa, fb))


def timed(fn, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn(batches)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(batches), res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=6, help="batches per round (default 6)")
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds after one warm-up round (default 5)")
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_outputs.log"))
    ap.add_argument("--append", action="store_true", help="add the report to --out as a new section instead of replacing the file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("tools/bench_infer_outputs.py needs the MI355X: there is no fallback and nothing to report without it", file=sys.stderr)
        return 2
    assert args.batches >= 2 and args.rounds >= 3
    lines = []

    def say(text: str = "") -> None:
        print(text, flush=True)
        lines.append(text)

    say(f"tools/bench_infer_outputs.py on one MI355X: decoded predictions [B, {5 + C}, {SY}, {SX}] ({IMG_H} x {IMG_W} images), {K} firing cells "
        f"per image; {args.batches} batches per round, {args.rounds} timed rounds after 1 warm-up round, host path and sink path alternating; "
        f"torch threads {torch.get_num_threads()}")
    say("milliseconds per batch: host clock around a round of one path, ending in a device synchronise; the sink path's round includes its "
        "final drain() / class_counts() and, for preds, the same text formatting and file writes as the host path; the preds text path "
        "ends in drain_text() (text formatted on the device) and the same number of file writes")
    below = text_below = True
    with tempfile.TemporaryDirectory(prefix="infer_outputs_") as tmp:
        for B in args.batch_sizes:
            batches = [make_preds(B, 500 + k) for k in range(2)]
            batches = [batches[i % 2] for i in range(args.batches)]
            say()
            say(f"B = {B}")
            for kind in ("count", "npy", "preds"):
                legs = Legs(kind, B, tmp)
                _, want = timed(legs.host, batches)          # warm-up round, and the check that the paths agree
                _, got = timed(legs.sink, batches)
                if not legs.same(want, got):
                    say(f"  {kind}: the two paths DISAGREE")
                    return 1
                if kind == "preds":
                    _, got_text = timed(legs.text, batches)
                    if not legs.same(want, got_text):
                        say("  preds: the text path DISAGREES with the host path")
                        return 1
                kept = {"count": lambda: sum(want), "npy": lambda: want.shape[1], "preds": lambda: -1}[kind]()
                th, ts, tt = [], [], []
                for _ in range(args.rounds):
                    th.append(timed(legs.host, batches)[0] * 1e3)
                    ts.append(timed(legs.sink, batches)[0] * 1e3)
                    if kind == "preds":
                        tt.append(timed(legs.text, batches)[0] * 1e3)
                below = below and all(s < h for h, s in zip(th, ts))
                text_below = text_below and all(t < s for s, t in zip(ts, tt))
                say(f"  {kind:5s} host path  " + " ".join(f"{v:9.3f}" for v in th) + f"   median {np.median(th):9.3f} ms   "
                    f"{legs.host_bytes / 1e6:10.3f} MB to the host per batch")
                say(f"  {kind:5s} sink path  " + " ".join(f"{v:9.3f}" for v in ts) + f"   median {np.median(ts):9.3f} ms   "
                    f"{legs.sink_bytes / 1e6:10.3f} MB to the host per batch   host / sink = {np.median(th) / np.median(ts):.1f}x"
                    + (f"   ({kept} kept rows per round)" if kept >= 0 else ""))
                if kind == "preds":
                    say(f"  {kind:5s} text path  " + " ".join(f"{v:9.3f}" for v in tt) + f"   median {np.median(tt):9.3f} ms   "
                        f"{legs.text_bytes / 1e6:10.3f} MB to the host per batch   sink / text = {np.median(ts) / np.median(tt):.1f}x")
                    say(f"        of which the file writes (open / write / close of {B} files per batch, host clock inside the text path's "
                        f"rounds): median {np.median(legs.write_ms[1:]):9.3f} ms")
                del legs
            del batches
            torch.cuda.empty_cache()
    say()
    say("the paths gave the same counts, the same .npy array and the same .txt bytes -- host, sink and text path for the latter -- "
        "(checked by the tool in the warm-up round)")
    say("sink path below the host path in every pair of rounds: " + ("yes" if below else "NO"))
    say("preds: text path (formatted on the device) below the sink path (formatted on the host) in every pair of rounds: "
        + ("yes" if text_below else "NO"))
    say("preds: what the text path still spends is the threshold + NMS launches, the append, one drain_text() and the file writes; the sink "
        "path's time above it is the host formatting (prediction_rows_to_text) and the larger read-back")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        if args.append and f.tell():
            f.write("\n" + "=" * 100 + "\n\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
